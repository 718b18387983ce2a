"""Kernel-level parity of the small kernels every SHOT-VAE step (configs 1-4) goes through, on a real MI355X: the heads
(sv_head_fwd / _bwd), the sampler (sv_sample_fwd / _bwd), the loss terms (sv_elbo_*, sv_cls_*, sv_post_*), the fused loss stage
(sv_shot_loss_step2, sv_shot_loss_step, sv_shot_targets, sv_shot_targets2, sv_shot_compose, sv_shot_scale), pairing and mixing
(sv_optimal_match, sv_mix_lerp) and the optimizers (sv_sgd, sv_adam), called directly through the C ABI.

Reference: float64 torch on the CPU, written from the formulas of oracle/shotvae_oracle.py (sample_latent, vae_criterion,
cls_criterion, pairwise_gaussian_kl, mix_with_index, the composition of train_step) and from torch.optim.SGD / Adam run in float64;
gradients are float64 autograd of that reference.  Inputs are drawn in fp32 (bf16 operands: rounded to bf16 first) and widened, so
both sides see the same operands; scalars the C ABI takes as `float` (lambda, the schedule, the optimizers' hyper-parameters) are
rounded to fp32 before the reference sees them.  Every output the kernel overwrites is pre-filled with NaN, outputs that accumulate
are pre-filled with non-zero values (the result must be old + gradient), and every buffer carries a guard tail that must stay as it
was.

Tolerances are not tuned to the kernels.  close(): for each quantity the same formula is restated in fp32 torch on the CPU and its
error against the float64 reference is measured on the test's own inputs (max |a - ref| / max |ref| over the tensor; the loss
terms and coefficients: the largest relative error of a single scalar); the kernel gets 8 x that error -- a different summation
order, float atomics, expf / logf an ulp off the host's.  Where the CPU's fp32 result is exact or lands nearer than half an fp32
ulp (2^-24) by chance -- single scalars, products of one rounding -- the measured error counts as 2^-24: no fp32 result can be
asked to be nearer than the format rounds.  bf16 outputs: within one bf16 ulp of the bf16 rounding of the reference.

Measured on the inputs below: the error of the CPU's fp32 restatement against float64 (what the allowance is 8 x of, case by
case), the kernel's on an MI355X, and the largest kernel error / allowance of any single check -- each the worst case of the
quantity over its cases, default and deterministic mode:

    quantity                       CPU fp32  kernel    worst kernel / allowance
    head mu                        3.8e-07   6.1e-07   0.20
    head ls                        4.0e-07   4.8e-07   0.19
    head la                        1.7e-07   2.8e-07   0.21
    head dfeat                     6.0e-07   1.0e-06   0.27
    head dout                      2.8e-07   8.4e-08   0.05
    head dW                        5.0e-07   4.3e-07   0.13
    head dbias                     1.3e-07   2.8e-07   0.31
    sample z                       1.1e-07   6.1e-08   0.07
    sample c                       1.0e-07   2.2e-07   0.27
    sample csoft                   1.0e-07   2.2e-07   0.27
    sample dmu                     5.6e-08   5.6e-08   0.12
    sample dls                     1.1e-07   1.1e-07   0.14
    sample dla                     8.9e-08   5.2e-08   0.09
    elbo terms                     1.2e-07   2.0e-07   0.43
    elbo dxr                       5.4e-07   5.4e-07   0.24
    elbo dmu                       5.1e-08   5.1e-08   0.11
    elbo dls                       1.2e-07   1.3e-07   0.16
    elbo dla                       8.9e-08   9.6e-08   0.14
    cls term                       4.6e-08   1.7e-07   0.37
    cls dpredict                   6.0e-08   4.8e-08   0.10
    post term                      9.7e-08   9.7e-08   0.12
    post dmu                       7.1e-08   7.1e-08   0.13
    post dls                       7.1e-08   7.7e-08   0.14
    stage terms                    1.7e-07   2.2e-07   0.23
    stage coef                     3.1e-08   3.1e-08   0.07
    stage tgt sm_mu                8.1e-08   8.1e-08   0.13
    stage tgt sm_sigma             1.0e-07   1.3e-07   0.20
    stage tgt mx_mu                7.5e-08   7.5e-08   0.13
    stage tgt mx_sigma             1.1e-07   1.1e-07   0.16
    stage tgt lab_mix              0.0e+00   0.0e+00   0.00
    stage tgt mx_alpha             9.3e-08   9.3e-08   0.13
    stage d_rec                    4.6e-07   4.6e-07   0.14
    stage d_mu                     1.1e-07   1.1e-07   0.13
    stage d_ls                     1.9e-07   1.9e-07   0.25
    stage d_la                     1.7e-07   1.3e-07   0.27
    compose losses                 4.2e-08   6.3e-08   0.13
    compose coef                   5.9e-08   5.9e-08   0.12
    scale gvec                     2.7e-08   2.7e-08   0.06
    targets sm_mu                  6.4e-08   6.4e-08   0.13
    targets sm_sigma               7.1e-08   8.2e-08   0.15
    targets lab_mix                0.0e+00   0.0e+00   0.00
    targets mx_mu                  5.5e-08   5.5e-08   0.11
    targets mx_sigma               8.1e-08   8.1e-08   0.13
    targets mx_alpha               5.1e-08   5.1e-08   0.11
    mix_lerp exp=0                 6.7e-08   6.1e-08   0.13
    mix_lerp exp=1                 8.4e-08   6.7e-08   0.12
    sgd p - p0                     4.8e-07   4.8e-07   0.25
    sgd v                          1.6e-07   9.3e-08   0.11
    adam p - p0                    1.5e-04   1.6e-04   0.13
    adam m (0, 1e-20, 1e4)         3.7e-07   2.2e-07   0.07
    adam v (0, 1e-20, 1e4)         9.5e-08   9.5e-08   0.13
    adam m (N(0,1))                1.1e-07   1.5e-07   0.22
    adam v (N(0,1))                1.6e-07   1.7e-07   0.17

    (adam p - p0: an Adam update is ~1e-3 of p, so the fp32 rounding of p itself is ~1e-4 of it.)
    sample csoft, the u = 0 / u = 1 row against the fp32 restatement: 2.0e-6 at K = 100 and 130, 2.3e-8 at K = 10; allowance
    1.5e-5 (8 x half an fp32 ulp of the softmax argument, |y| up to 41).
    sv_optimal_match: margin = 20 x the fp32 KL error = 2.7e-4 (B = 2) ... 5.6e-3 (D = 512) against KL values of 72 ... 667; no
    row of the five cases has a float64 gap below its margin.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from shot_vae_amd import _lib as L          # noqa: E402
from oracle import shotvae_oracle as O      # noqa: E402

DT = {"f32": (L.SV_F32, torch.float32), "bf16": (L.SV_BF16, torch.bfloat16)}
NAN = float("nan")
HALF_ULP = 2.0 ** -24
GUARD = 2                        # extra rows (1-D buffers: elements) behind every buffer a kernel writes
SV_E_SHAPE = -2                  # include/shotvae_hip.h
F64, F32 = torch.float64, torch.float32


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
    assert t.is_cuda and t.is_contiguous()
    _KEEP.append(t)
    if len(_KEEP) > 4096:
        torch.cuda.synchronize()
        del _KEEP[:2048]
    return C.c_void_p(t.data_ptr())


def rel(a, b, each=False):
    """max |a - b| / max |b|; each: the largest relative error of a single element"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    d = (a - b).abs()
    if each:
        return float((d / b.abs().clamp_min(1e-30)).max())
    return float(d.max() / b.abs().max().clamp_min(1e-30))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32v(v):
    """the value a `float` argument of the C ABI carries"""
    return float(torch.tensor(float(v), dtype=F32))


def buf(rows, *cols, fill=NAN, dtype=F32):
    """[rows + GUARD, *cols] on the device, filled (NaN: an element the kernel does not write fails the test)"""
    return torch.full((rows + GUARD,) + tuple(cols), fill, dtype=dtype, device=dev())


def filled(t, dtype=None):
    """t with a NaN guard tail, on the device"""
    t = t if dtype is None else t.to(dtype)
    b = buf(t.shape[0], *t.shape[1:], dtype=t.dtype)
    b[:t.shape[0]] = t.to(dev())
    return b


def tail_untouched(t, rows, what):
    assert torch.isnan(t[rows:].float()).all(), what + ": guard tail written"


def allowance(f32, ref, each=False):
    return 8.0 * max(rel(f32, ref, each), HALF_ULP)


def close(got, f32, ref, what, each=False):
    """kernel result within 8 x the error of the CPU's fp32 restatement (module docstring); prints the three figures"""
    got = got.detach().float().cpu()
    assert not torch.isnan(got).any(), what + ": NaN left (element not written)"
    cpu, e, lim = rel(f32, ref, each), rel(got, ref, each), allowance(f32, ref, each)
    print("FIG %-34s cpu32 %.3e kernel %.3e allow %.3e" % (what, cpu, e, lim))
    assert e <= lim, "%s: kernel error %g > 8 x the fp32 restatement's %g" % (what, e, cpu)


def bf16_ulp(x):
    """spacing of bf16 at |x| (8 significant bits); 0 at 0"""
    a = x.abs().double()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -126)))
    return torch.where(a > 0, torch.exp2(e - 7), torch.zeros_like(a))


def assert_bf16(got, ref, floor, what):
    """got (bf16) within one bf16 ulp of bf16(ref); `floor` absorbs the fp32 rounding of the kernel's own arithmetic where a
    value is far below the tensor's scale (an ulp of such a value is below that rounding)"""
    assert got.dtype == torch.bfloat16
    got = got.double().cpu()
    assert not torch.isnan(got).any(), what + ": NaN left (element not written)"
    r = ref.to(torch.bfloat16).double()
    err = (got - r).abs()
    lim = bf16_ulp(torch.maximum(r.abs(), got.abs())) + floor
    bad = err > lim
    assert not bad.any(), "%s: %d elements beyond 1 bf16 ulp, worst %g (got %g, want %g)" % (
        what, int(bad.sum()), float(err.max()), float(got[bad][0]), float(r[bad][0]))


def check(got, f32, ref, dt, what):
    """fp32 outputs: close(); bf16 outputs: the one-ulp rule, the floor being the fp32 allowance in absolute terms"""
    if dt == "bf16":
        assert_bf16(got.cpu(), ref, allowance(f32, ref) * float(ref.abs().max()), what)
    else:
        close(got, f32, ref, what)


# ------------------------------------------------------------------------------------------------ 1. heads
# (C, ldc, K, B): the thread-group split that meets in LDS (C < 256, 256 % C == 0; B % 4 != 0) | C < 256 that does not divide 256:
# the general loop, one blockIdx.y | two 256-channel slices, the second 128-sample weight slice holds ONE sample | three channel
# slices (the last partial), K > 64 (strided log-softmax), NH = 356 is no multiple of 32, two weight slices | a full block
HEAD_SHAPES = [(128, 128, 10, 5), (96, 128, 10, 6), (512, 128, 10, 129), (640, 128, 100, 130), (64, 64, 10, 4)]


def _head_math(feat, W, bias, ups, old, ldc, K):
    """vae_forward's heads (oracle/shotvae_oracle.py: three F.linear on the pooled features, log_softmax on the last K) and the
    gradients of sum(out * upstream) by autograd; W = [mean | log_sigma | disc] rows, [2 ldc + K][C]"""
    dt = feat.dtype
    feat, W, bias = (t.clone().requires_grad_(True) for t in (feat, W, bias))
    o = F.linear(feat, W, bias)
    mu, ls, la = o[:, :ldc], o[:, ldc:2 * ldc], F.log_softmax(o[:, 2 * ldc:], dim=1)
    loss = (mu * ups[0].to(dt)).sum() + (ls * ups[1].to(dt)).sum() + (la * ups[2].to(dt)).sum()
    dfeat, dW, db, do = torch.autograd.grad(loss, [feat, W, bias, o])
    return dict(mu=mu.detach(), ls=ls.detach(), la=la.detach(), dfeat=dfeat, dout=do, dW=old[0].to(dt) + dW, dbias=old[1].to(dt) + db)


@functools.lru_cache(maxsize=None)
def _head_case(Cc, ldc, K, B):
    g = gen(1000 + Cc + B)
    NH = 2 * ldc + K
    I = dict(feat=torch.randn(B, Cc, generator=g), W=torch.randn(NH, Cc, generator=g) / Cc ** 0.5,
             bias=0.1 * torch.randn(NH, generator=g),
             ups=(torch.randn(B, ldc, generator=g), torch.randn(B, ldc, generator=g), torch.randn(B, K, generator=g)),
             old=(torch.randn(NH, Cc, generator=g), torch.randn(NH, generator=g)))
    r64 = _head_math(I["feat"].double(), I["W"].double(), I["bias"].double(), I["ups"], I["old"], ldc, K)
    r32 = _head_math(I["feat"], I["W"], I["bias"], I["ups"], I["old"], ldc, K)
    return I, r64, r32


def _head_run(I, la_saved, Cc, ldc, K, B):
    """sv_head_fwd + sv_head_bwd -> the device buffers (guard tails included)"""
    NH = 2 * ldc + K
    d = dev()
    feat, W, bias = I["feat"].to(d), I["W"].to(d), I["bias"].to(d)
    out = dict(mu=buf(B, ldc), ls=buf(B, ldc), la=buf(B, K))
    L.call("sv_head_fwd", p(feat), B, Cc, p(W), p(bias), ldc, K, p(out["mu"]), p(out["ls"]), p(out["la"]), st())
    out.update(dfeat=buf(B, Cc), dout=buf(B, NH), dW=filled(I["old"][0]), dbias=filled(I["old"][1]))
    ups = [t.to(d) for t in I["ups"]]
    L.call("sv_head_bwd", p(feat), B, Cc, p(W), ldc, K, p(la_saved.float().to(d)), p(ups[0]), p(ups[1]), p(ups[2]),
           p(out["dfeat"]), p(out["dW"]), p(out["dbias"]), p(out["dout"]), st())
    torch.cuda.synchronize()
    return out


def _head_check(out, r64, r32, Cc, ldc, K, B, tag):
    NH = 2 * ldc + K
    rows = dict(mu=B, ls=B, la=B, dfeat=B, dout=B, dW=NH, dbias=NH)
    for k, n in rows.items():
        close(out[k][:n], r32[k], r64[k], "head %s %s" % (k, tag))
        tail_untouched(out[k], n, "head %s %s" % (k, tag))


@pytest.mark.parametrize("Cc,ldc,K,B", HEAD_SHAPES)
def test_head_fwd_bwd_against_float64(Cc, ldc, K, B):
    I, r64, r32 = _head_case(Cc, ldc, K, B)
    out = _head_run(I, r64["la"], Cc, ldc, K, B)
    _head_check(out, r64, r32, Cc, ldc, K, B, "C=%d" % Cc)


def test_head_bwd_deterministic_mode():
    """the 128-sample weight slices launched one after the other: the same tolerance, and two runs bit-equal"""
    Cc, ldc, K, B = HEAD_SHAPES[3]
    I, r64, r32 = _head_case(Cc, ldc, K, B)
    with L.options(deterministic=1):                 # (restores the option on exit, also when the block raises)
        a = _head_run(I, r64["la"], Cc, ldc, K, B)
        b = _head_run(I, r64["la"], Cc, ldc, K, B)
    assert not L.deterministic()
    _head_check(a, r64, r32, Cc, ldc, K, B, "C=%d det" % Cc)
    NH = 2 * ldc + K
    for k, n in (("dfeat", B), ("dout", B), ("dW", NH), ("dbias", NH)):
        assert torch.equal(a[k][:n], b[k][:n]), k + ": deterministic mode is not reproducible"


# ------------------------------------------------------------------------------------------------ 2. sampler
# (ldc, K, Lpad, B): the base case | K > 64: both waves of the max / sum reduction hold classes | K > 128: the strided loops take a
# second trip; ldc no multiple of the 128-thread block
SAMPLE_SHAPES = [(128, 10, 144, 3), (128, 100, 240, 3), (200, 130, 336, 2)]
TEMP = f32v(0.67)
LAM = f32v(0.3)


@functools.lru_cache(maxsize=None)
def _sample_inputs(ldc, K, B):
    """B ordinary rows + one edge row (u = 0 and u = 1 exactly, alternating)"""
    g = gen(2000 + ldc + K)
    Bt = B + 1
    u = (2.0 ** -20 + torch.rand(Bt, K, generator=g) * (1.0 - 2.0 ** -19)).clamp(2.0 ** -20, 1.0 - 2.0 ** -20)
    u[B] = (torch.arange(K) % 2).float()
    return dict(mu=torch.randn(Bt, ldc, generator=g), ls=0.3 * torch.randn(Bt, ldc, generator=g),
                la=F.log_softmax(1.5 * torch.randn(Bt, K, generator=g), dim=1), eps=torch.randn(Bt, ldc, generator=g), u=u,
                label=torch.randint(0, K, (Bt,), generator=g), label_mix=torch.randint(0, K, (Bt,), generator=g))


def _sample_math(I, mode, dt, rows, dlat=None):
    """oracle sample_latent in dtype dt on the first `rows` rows -> latent [rows][ldc + K] (and, with dlat, the gradients of
    sum(latent * dlat) w.r.t. mu, log_sigma, log_alpha; None where the latent does not depend on the input)"""
    mu, ls, la = (I[k][:rows].to(dt).requires_grad_(dlat is not None) for k in ("mu", "ls", "la"))
    eps = I["eps"][:rows].to(dt)
    if mode == 0:
        lat = O.sample_latent(mu, ls, la, eps, u=I["u"][:rows].to(dt), temperature=TEMP)
    else:
        lat = O.sample_latent(mu, ls, la, eps, label=I["label"][:rows], mixup=mode == 2, label_mix=I["label_mix"][:rows], lam=LAM,
                              temperature=TEMP)
    lat = lat[:, :, 0, 0]
    if dlat is None:
        return lat
    grads = torch.autograd.grad((lat * dlat[:rows, :lat.shape[1]].to(dt)).sum(), [mu, ls, la], allow_unused=True)
    return lat.detach(), grads


@pytest.mark.parametrize("ldc,K,Lpad,B", SAMPLE_SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2, "2dev"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sample_fwd_against_float64(dt, mode, ldc, K, Lpad, B):
    code, tdt = DT[dt]
    d = dev()
    I = _sample_inputs(ldc, K, B)
    Bt = B + 1
    lam_dev = None
    lam = LAM
    if mode == "2dev":                          # lambda through the device pointer; the by-value argument is poisoned
        mode, lam, lam_dev = 2, -7.0, torch.tensor([LAM], device=d)
    if mode == 1:
        lam = -7.0                              # unused without mixup
    r64 = _sample_math(I, mode, F64, B)
    r32 = _sample_math(I, mode, F32, Bt)
    latent, csoft = buf(Bt, Lpad, dtype=tdt), buf(Bt, K)
    g = {k: I[k].to(d) for k in I}
    L.call("sv_sample_fwd", code, p(g["mu"]), p(g["ls"]), p(g["la"]), p(g["eps"]), p(g["u"]) if mode == 0 else None,
           None if mode == 0 else p(g["label"]), p(g["label_mix"]) if mode == 2 else None, lam, p(lam_dev), mode, TEMP, Bt, ldc, K,
           Lpad, p(latent), p(csoft), st())
    torch.cuda.synchronize()
    tag = "K=%d mode %d %s" % (K, mode, dt)
    lat, cs = latent.cpu(), csoft.cpu()
    check(latent[:B, :ldc], r32[:B, :ldc], r64[:, :ldc], dt, "sample z " + tag)
    check(latent[:B, ldc:ldc + K], r32[:B, ldc:], r64[:, ldc:], dt, "sample c " + tag)
    close(csoft[:B], r32[:B, ldc:], r64[:, ldc:], "sample csoft " + tag)
    # the edge row (u = 0 / u = 1): the float64 formula is no reference there (its 1e-12 terms do not round away) -- finite, and
    # the fp32 restatement of sample_latent.  Allowance: c = softmax(y), y = (log_alpha + gumbel) / T, so an absolute change of
    # y_k is the same relative change of c_k.  On this row gumbel = -log(1e-12) = 27.6 and |y| reaches ~45, where fp32 rounds y
    # to multiples of 2^-18: a host logf one ulp off the device's moves every y_k to another grid point.  The rounding unit of y
    # (half an ulp at max |y|) takes the place of the measured error of the ordinary rows (|y| mostly below 4) where it is larger.
    assert torch.isfinite(lat[B].float()).all() and torch.isfinite(cs[B]).all()
    e, lim = rel(cs[B], r32[B, ldc:]), allowance(r32[:B, ldc:], r64[:, ldc:])
    if mode == 0:
        gum = -torch.log(-torch.log(I["u"][B] + O.GUMBEL_EPS) + O.GUMBEL_EPS)
        ymax = float(((I["la"][B] + gum) / TEMP).abs().max())
        lim = max(lim, 8.0 * 2.0 ** (math.floor(math.log2(ymax)) - 24))
    print("FIG %-34s kernel %.3e allow %.3e" % ("sample csoft edge row " + tag, e, lim))
    assert e <= lim, "csoft, edge row: %g > %g" % (e, lim)
    assert torch.equal(lat[:Bt, ldc + K:].float(), torch.zeros(Bt, Lpad - ldc - K)), "latent pad columns must be 0"
    assert torch.equal(lat[:Bt, ldc:ldc + K], cs[:Bt].to(tdt)), "csoft is not the fp32 value whose rounding is in latent"
    tail_untouched(latent, Bt, "latent")
    tail_untouched(csoft, Bt, "csoft")


@pytest.mark.parametrize("ldc,K,Lpad,B", SAMPLE_SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sample_bwd_against_float64_autograd(dt, mode, ldc, K, Lpad, B):
    code, tdt = DT[dt]
    d = dev()
    I = _sample_inputs(ldc, K, B)
    g = gen(2100 + K + mode)
    dlat = torch.randn(B, Lpad, generator=g).to(tdt)              # (bf16: rounded before it reaches the reference)
    old = [torch.randn(B, n, generator=g) for n in (ldc, ldc, K)]
    lat64, g64 = _sample_math(I, mode, F64, B, dlat.float())
    _, g32 = _sample_math(I, mode, F32, B, dlat.float())
    dl = dlat.clone()
    dl[:, ldc + K:] = NAN                                            # pad columns: garbage that must not leak
    outs = [filled(t) for t in old]
    csoft = lat64[:, ldc:].float().to(d)                             # the saved sample, rounded to fp32
    L.call("sv_sample_bwd", code, p(dl.to(d)), p(I["ls"][:B].to(d)), p(I["eps"][:B].to(d)), p(csoft), mode, TEMP, B, ldc, K, Lpad,
           p(outs[0]), p(outs[1]), p(outs[2]), st())
    torch.cuda.synchronize()
    for name, o, prev, a64, a32 in zip(("dmu", "dls", "dla"), outs, old, g64, g32):
        what = "sample %s K=%d mode %d %s" % (name, K, mode, dt)
        if a64 is None:
            assert name == "dla" and mode != 0
            assert torch.equal(o[:B].cpu(), prev), "dla must be left untouched in modes 1 and 2"
        else:
            close(o[:B], prev + a32, prev.double() + a64, what)              # accumulates: old + gradient
        tail_untouched(o, B, what)


# ------------------------------------------------------------------------------------------------ 3. loss terms
# (B, n_per_img, ldc, K): n = 225, the scalar tail behind the 16-byte loop | one block, the latent loops stride 20 times | 6 blocks
ELBO_SHAPES = [(3, 75, 128, 10), (40, 64, 128, 100), (7, 3072, 128, 10)]
X_SIGMA = 0.5                    # (exact in fp32)
GOUT3 = (0.7, -1.3, 2.1)


def _elbo_math(I, bce, dt):
    x, xr, mu, ls, la = (I[k].to(dt) for k in ("x", "xr", "mu", "ls", "la"))
    xr, mu, ls, la = (t.requires_grad_(True) for t in (xr, mu, ls, la))
    terms = torch.stack(O.vae_criterion(x, xr, mu, ls, la, X_SIGMA, bool(bce)))          # log_prior: log(float32(1 / K)) in float32
    gw = torch.tensor([f32v(v) for v in GOUT3], dtype=dt)
    grads = torch.autograd.grad((terms * gw).sum(), [xr, mu, ls, la])
    return terms.detach(), grads


@functools.lru_cache(maxsize=None)
def _elbo_case(B, npi, ldc, K, bce, wide):
    g = gen(3000 + B + npi + K)
    xr = 2.0 * torch.randn(B, npi, generator=g)
    if wide:                     # |x_rec| up to 30: exp(-|x|) down to 1e-13, the stable form of BCE
        xr = 30.0 * (2.0 * torch.rand(B, npi, generator=g) - 1.0)
        xr[0, :2] = torch.tensor([30.0, -30.0])
    I = dict(x=torch.rand(B, npi, generator=g), xr=xr, mu=0.7 * torch.randn(B, ldc, generator=g),
             ls=0.3 * torch.randn(B, ldc, generator=g) - 0.5, la=F.log_softmax(2.0 * torch.randn(B, K, generator=g), dim=1))
    return I, _elbo_math(I, bce, F64), _elbo_math(I, bce, F32)


def _elbo_run(I, B, npi, ldc, K, bce, backward=True):
    d = dev()
    x, xr, mu, ls, la = (I[k].to(d) for k in ("x", "xr", "mu", "ls", "la"))
    out3 = buf(3)
    out3[:3] = 0.0                                                    # (the terms accumulate: zeroed by the caller)
    args = [p(x), p(xr), npi, p(mu), p(ls), p(la), B, ldc, K, bce, X_SIGMA]
    L.call("sv_elbo_fwd", *args, p(out3), st())
    grads = [buf(B, npi), buf(B, ldc), buf(B, ldc), buf(B, K)]
    if backward:
        gout = torch.tensor([f32v(v) for v in GOUT3], device=d)
        L.call("sv_elbo_bwd", *args, p(gout), *[p(t) for t in grads], st())
    torch.cuda.synchronize()
    return out3, grads


@pytest.mark.parametrize("B,npi,ldc,K", ELBO_SHAPES)
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("bce", [1, 0])
def test_elbo_against_float64(bce, wide, B, npi, ldc, K):
    I, (t64, g64), (t32, g32) = _elbo_case(B, npi, ldc, K, bce, wide)
    out3, grads = _elbo_run(I, B, npi, ldc, K, bce)
    tag = "bce=%d n=%d K=%d%s" % (bce, B * npi, K, " wide" if wide else "")
    close(out3[:3], t32, t64, "elbo terms " + tag, each=True)
    tail_untouched(out3, 3, "out3")
    for name, o, a64, a32 in zip(("dxr", "dmu", "dls", "dla"), grads, g64, g32):
        close(o[:B], a32, a64, "elbo %s %s" % (name, tag))
        tail_untouched(o, B, "elbo " + name)


def _cls_math(I, dt, weighted):
    pred = I["pred"].to(dt).requires_grad_(True)
    out = O.cls_criterion(pred, I["label"].to(dt), I["w"].to(dt) if weighted else None)
    grad, = torch.autograd.grad(out * f32v(0.8), pred)
    return out.detach().view(1), grad


@functools.lru_cache(maxsize=None)
def _cls_case(B, K, weighted):
    g = gen(3100 + B)
    I = dict(pred=F.log_softmax(2.0 * torch.randn(B, K, generator=g), dim=1), label=F.softmax(torch.randn(B, K, generator=g), dim=1),
             w=torch.rand(B, generator=g))
    return I, _cls_math(I, F64, weighted), _cls_math(I, F32, weighted)


def _cls_run(I, B, K, weighted, backward=True):
    d = dev()
    pred, label, w = I["pred"].to(d), I["label"].to(d), I["w"].to(d) if weighted else None
    out = buf(1)
    out[:1] = 0.0
    L.call("sv_cls_fwd", p(pred), p(label), p(w), B, K, p(out), st())
    dp = buf(B, K)
    if backward:
        L.call("sv_cls_bwd", p(label), p(w), B, K, p(torch.tensor([f32v(0.8)], device=d)), p(dp), st())
    torch.cuda.synchronize()
    return out, dp


@pytest.mark.parametrize("B,K", [(200, 100), (5, 10)])            # 20 000 elements: past the 64-block cap (grid-stride loop) | one block
@pytest.mark.parametrize("weighted", [0, 1])
def test_cls_against_float64(weighted, B, K):
    I, (t64, g64), (t32, g32) = _cls_case(B, K, weighted)
    out, dp = _cls_run(I, B, K, weighted)
    tag = "B=%d w=%d" % (B, weighted)
    close(out[:1], t32, t64, "cls term " + tag, each=True)
    close(dp[:B], g32, g64, "cls dpredict " + tag)
    tail_untouched(out, 1, "cls out")
    tail_untouched(dp, B, "cls dpredict")


def _post_math(I, dt):
    """train_step's cont_post: (sum (mu - mu_t)^2 + sum (exp(log_sigma) - sigma_t)^2) / B"""
    mu, ls = (I[k].to(dt).requires_grad_(True) for k in ("mu", "ls"))
    mt, s_t = I["mt"].to(dt), I["st"].to(dt)
    out = (((mu - mt) ** 2).sum() + ((torch.exp(ls) - s_t) ** 2).sum()) / mu.shape[0]
    grads = torch.autograd.grad(out * f32v(0.8), [mu, ls])
    return out.detach().view(1), grads


@functools.lru_cache(maxsize=None)
def _post_case(B, D):
    g = gen(3200 + B)
    I = dict(mu=0.7 * torch.randn(B, D, generator=g), ls=0.3 * torch.randn(B, D, generator=g) - 0.5,
             mt=torch.randn(B, D, generator=g), st=torch.rand(B, D, generator=g) + 0.2)
    return I, _post_math(I, F64), _post_math(I, F32)


def _post_run(I, B, D, backward=True):
    d = dev()
    mu, ls, mt, s_t = (I[k].to(d) for k in ("mu", "ls", "mt", "st"))
    out = buf(1)
    out[:1] = 0.0
    L.call("sv_post_fwd", p(mu), p(ls), p(mt), p(s_t), B, D, p(out), st())
    dmu, dls = buf(B, D), buf(B, D)
    if backward:
        L.call("sv_post_bwd", p(mu), p(ls), p(mt), p(s_t), B, D, p(torch.tensor([f32v(0.8)], device=d)), p(dmu), p(dls), st())
    torch.cuda.synchronize()
    return out, dmu, dls


@pytest.mark.parametrize("B,D", [(130, 128), (3, 100)])            # 16 640 elements: past the 64-block cap | two blocks, a partial one
def test_post_against_float64(B, D):
    I, (t64, g64), (t32, g32) = _post_case(B, D)
    out, dmu, dls = _post_run(I, B, D)
    close(out[:1], t32, t64, "post term B=%d" % B, each=True)
    close(dmu[:B], g32[0], g64[0], "post dmu B=%d" % B)
    close(dls[:B], g32[1], g64[1], "post dls B=%d" % B)
    tail_untouched(out, 1, "post out")
    tail_untouched(dmu, B, "post dmu")
    tail_untouched(dls, B, "post dls")


def test_loss_terms_deterministic_mode():
    """one multi-block case of each forward through the per-block slots + the in-order collection: the same tolerance, two runs
    bit-equal"""
    B, npi, ldc, K = ELBO_SHAPES[2]
    Ie, (e64, _), (e32, _) = _elbo_case(B, npi, ldc, K, 1, 0)
    Ic, (c64, _), (c32, _) = _cls_case(200, 100, 1)
    Ip, (p64, _), (p32, _) = _post_case(130, 128)
    runs = []
    with L.options(deterministic=1):
        for _ in range(2):
            runs.append((_elbo_run(Ie, B, npi, ldc, K, 1, backward=False)[0], _cls_run(Ic, 200, 100, 1, backward=False)[0],
                         _post_run(Ip, 130, 128, backward=False)[0]))
    assert not L.deterministic()
    for a, b in zip(*runs):
        assert torch.equal(a[:-GUARD], b[:-GUARD]), "deterministic mode is not reproducible"
    close(runs[0][0][:3], e32, e64, "elbo terms det", each=True)
    close(runs[0][1][:1], c32, c64, "cls term det", each=True)
    close(runs[0][2][:1], p32, p64, "post term det", each=True)


# ------------------------------------------------------------------------------------------------ 4. fused loss stage
SCH_KEYS = ("ew", "kl_beta_c", "kl_beta_d", "cmi", "dmi", "pwm", "ucw")
LEAVES = ("rec1", "mu1", "ls1", "la1", "rec3", "mu3", "ls3", "la3", "mu2", "ls2", "la2", "mu4", "ls4", "la4")
LAM_L, LAM_U = f32v(0.83), f32v(0.37)


def _sched(sch):
    return L.SvShotSchedule(*[sch[k] for k in SCH_KEYS])


def _targets_math(mu1, ls1, mu3, ls3, la3, label, perm_l, perm_u, K, dt):
    """the (detached) targets of the mixed forwards: mix_with_index on the outputs of forwards (1) and (3), and the soft label
    lam * onehot(y) + (1 - lam) * onehot(y[perm]) (cls_criterion is linear in its label, train_step's two label terms)"""
    with torch.no_grad():
        _, sm_mu, sm_sigma, _ = O.mix_with_index(mu1, mu1, ls1, ls1, LAM_L, perm_l)
        _, mx_mu, mx_sigma, mx_alpha = O.mix_with_index(mu3, mu3, ls3, la3, LAM_U, perm_u)
        oh = F.one_hot(label, K).to(dt)
        lab_mix = LAM_L * oh + (1 - LAM_L) * F.one_hot(label[perm_l], K).to(dt)
    return dict(sm_mu=sm_mu, sm_sigma=sm_sigma, mx_mu=mx_mu, mx_sigma=mx_sigma, lab_mix=lab_mix, mx_alpha=mx_alpha)


def _stage_math(I, sch, bce, dt):
    """the loss stage of oracle train_step (the criteria of forwards (1), (3), the targets, the posterior terms of (2), (4), the two
    objectives) in dtype dt -> (terms[12], coef[10] = d(loss_sup + loss_unsup) / d term, targets, gradients w.r.t. LEAVES)"""
    v = {k: I[k].to(dt).requires_grad_(True) for k in LEAVES}
    il, iu, label, perm_l, perm_u = I["il"].to(dt), I["iu"].to(dt), I["label"], I["perm_l"], I["perm_u"]
    Bl, Bu, K = il.shape[0], iu.shape[0], I["la1"].shape[1]
    recon_l, klc_l, kld_l = O.vae_criterion(il, v["rec1"], v["mu1"], v["ls1"], v["la1"], X_SIGMA, bool(bce))
    recon_u, klc_u, kld_u = O.vae_criterion(iu, v["rec3"], v["mu3"], v["ls3"], v["la3"], X_SIGMA, bool(bce))
    T = _targets_math(v["mu1"], v["ls1"], v["mu3"], v["ls3"], v["la3"], label, perm_l, perm_u, K, dt)
    oh = F.one_hot(label, K).to(dt)
    disc_post_l = LAM_L * O.cls_criterion(v["la2"], oh) + (1 - LAM_L) * O.cls_criterion(v["la2"], F.one_hot(label[perm_l], K).to(dt))
    cont_post_l = (((v["mu2"] - T["sm_mu"]) ** 2).sum() + ((torch.exp(v["ls2"]) - T["sm_sigma"]) ** 2).sum()) / Bl
    disc_post_u = O.cls_criterion(v["la4"], T["mx_alpha"])
    cont_post_u = (((v["mu4"] - T["mx_mu"]) ** 2).sum() + ((torch.exp(v["ls4"]) - T["mx_sigma"]) ** 2).sum()) / Bu
    elbo_l = recon_l + sch["kl_beta_c"] * torch.abs(klc_l - sch["cmi"]) + sch["kl_beta_d"] * torch.abs(kld_l - sch["dmi"])
    elbo_l = elbo_l + sch["kl_beta_c"] * sch["pwm"] * cont_post_l
    loss_sup = sch["ew"] * elbo_l + disc_post_l
    elbo_u = recon_u + sch["kl_beta_c"] * torch.abs(klc_u - sch["cmi"]) + sch["kl_beta_d"] * torch.abs(kld_u - sch["dmi"])
    elbo_u = elbo_u + sch["kl_beta_c"] * sch["pwm"] * cont_post_u
    loss_unsup = sch["ew"] * elbo_u + sch["ucw"] * disc_post_u
    raw = [recon_l, klc_l, kld_l, recon_u, klc_u, kld_u, disc_post_l, cont_post_l, disc_post_u, cont_post_u]
    grads = torch.autograd.grad(loss_sup + loss_unsup, raw + [v[k] for k in LEAVES])
    terms = torch.stack([t.detach() for t in raw + [loss_sup, loss_unsup]])
    return terms, torch.stack(grads[:10]), T, dict(zip(LEAVES, grads[10:]))


@functools.lru_cache(maxsize=None)
def _stage_case(Bl, Bu, K, bce, npi):
    D = 128
    g = gen(4000 + 31 * Bl + Bu + K + npi)
    I = dict(il=torch.rand(Bl, npi, generator=g), iu=torch.rand(Bu, npi, generator=g), label=torch.randint(0, K, (Bl,), generator=g),
             perm_l=torch.randperm(Bl, generator=g), perm_u=torch.randperm(Bu, generator=g))
    for i, B in ((1, Bl), (2, Bl), (3, Bu), (4, Bu)):
        I["mu%d" % i] = 0.5 * torch.randn(B, D, generator=g)
        I["ls%d" % i] = 0.3 * torch.randn(B, D, generator=g)
        I["la%d" % i] = F.log_softmax(torch.randn(B, K, generator=g), dim=1)
        if i in (1, 3):
            I["rec%d" % i] = torch.randn(B, npi, generator=g)
    sch = {k: f32v(v) for k, v in O.schedule(37, dmi=2.3).items()}
    r64 = _stage_math(I, sch, bce, F64)
    # (the signs of KL - capacity are well away from 0, or no fp32 computation could be asked to agree with float64)
    assert float((r64[0][[1, 4]] - sch["cmi"]).abs().min()) > 1e-2 and float((r64[0][[2, 5]] - sch["dmi"]).abs().min()) > 1e-2
    return I, sch, r64, _stage_math(I, sch, bce, F32)


TGT_ORDER = ("sm_mu", "sm_sigma", "mx_mu", "mx_sigma", "lab_mix", "mx_alpha")


def _stage_check(terms, coef, tgt, T64, T32, got, r64, r32, tag):
    close(terms, r32[0], r64[0], "stage terms " + tag, each=True)
    close(coef, r32[1], r64[1], "stage coef " + tag, each=True)
    o = 0
    for k in TGT_ORDER:
        n = T64[k].numel()
        close(tgt[o:o + n].view(T64[k].shape), T32[k], T64[k], "stage tgt %s %s" % (k, tag))
        o += n
    for k in LEAVES:
        close(got[k], r32[3][k], r64[3][k], "stage d_%s %s" % (k, tag))


@pytest.mark.parametrize("Bl,Bu", [(24, 24), (5, 24), (24, 7)])
@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("bce", [1, 0])
@pytest.mark.parametrize("npi", [3072, 75])
@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("lam_dev", [0, 1])
def test_shot_loss_step2_against_float64_stage(lam_dev, det, npi, bce, K, Bl, Bu):
    D = 128
    d = dev()
    I, sch, r64, r32 = _stage_case(Bl, Bu, K, bce, npi)
    g = {k: I[k].to(d) for k in I}
    grads = {k: buf(I[k].shape[0], I[k].shape[1]) for k in LEAVES}           # every per-group buffer with its own guard tail
    ntgt = 2 * (Bl + Bu) * D + (Bl + Bu) * K
    terms, coef, tgt = buf(12), buf(10), buf(ntgt)
    terms[:12] = 0.0
    a = L.SvShotLossArgs2()
    for slot, i in enumerate((1, 3, 2, 4)):                                   # the library's group order
        a.mu[slot], a.ls[slot], a.la[slot] = (g["%s%d" % (n, i)].data_ptr() for n in ("mu", "ls", "la"))
        a.d_mu[slot], a.d_ls[slot], a.d_la[slot] = (grads["%s%d" % (n, i)].data_ptr() for n in ("mu", "ls", "la"))
    for slot, i in enumerate((1, 3)):
        a.rec[slot], a.d_rec[slot] = g["rec%d" % i].data_ptr(), grads["rec%d" % i].data_ptr()
    a.image_l, a.image_u, a.label_l = g["il"].data_ptr(), g["iu"].data_ptr(), g["label"].data_ptr()
    a.perm_l, a.perm_u = g["perm_l"].data_ptr(), g["perm_u"].data_ptr()
    lams = torch.tensor([LAM_L, LAM_U], device=d)
    if lam_dev:                                                                # the by-value lambdas are poisoned
        a.lam_l, a.lam_u, a.lam_l_dev, a.lam_u_dev = -3.0, 5.0, lams.data_ptr(), lams.data_ptr() + 4
    else:
        a.lam_l, a.lam_u = LAM_L, LAM_U
    a.Bl, a.Bu, a.D, a.K, a.bce, a.n_per_img, a.x_sigma = Bl, Bu, D, K, bce, npi, X_SIGMA
    a.sch = _sched(sch)
    a.terms, a.coef, a.tgt = terms.data_ptr(), coef.data_ptr(), tgt.data_ptr()
    with L.options(deterministic=det):
        L.call("sv_shot_loss_step2", C.byref(a), st())
    torch.cuda.synchronize()
    tag = "Bl=%d Bu=%d K=%d bce=%d n=%d det=%d" % (Bl, Bu, K, bce, npi, det)
    _stage_check(terms[:12], coef[:10], tgt[:ntgt], r64[2], r32[2], {k: grads[k][:I[k].shape[0]] for k in LEAVES}, r64, r32, tag)
    for k in LEAVES:
        tail_untouched(grads[k], I[k].shape[0], "d_" + k)
    for t, n, what in ((terms, 12, "terms"), (coef, 10, "coef"), (tgt, ntgt, "tgt")):
        tail_untouched(t, n, what)


def test_shot_loss_step_batched_form_against_float64_stage():
    """sv_shot_loss_step: the four groups of one batched launch back to back in the order (1)(3)(2)(4)"""
    B, D, K, bce, npi = 24, 128, 10, 1, 75
    d = dev()
    I, sch, r64, r32 = _stage_case(B, B, K, bce, npi)
    cat = lambda n, ids: torch.cat([I["%s%d" % (n, i)] for i in ids]).to(d)
    rec, mu, ls, la = cat("rec", (1, 3)), cat("mu", (1, 3, 2, 4)), cat("ls", (1, 3, 2, 4)), cat("la", (1, 3, 2, 4))
    g = [buf(t.shape[0], t.shape[1]) for t in (rec, mu, ls, la)]
    ntgt = 4 * B * D + 2 * B * K
    terms, coef, tgt = buf(12), buf(10), buf(ntgt)
    terms[:12] = 0.0
    keep = [I[k].to(d) for k in ("il", "iu", "label", "perm_l", "perm_u")]
    a = L.SvShotLossArgs()
    a.rec, a.mu, a.ls, a.la = (t.data_ptr() for t in (rec, mu, ls, la))
    a.d_rec, a.d_mu, a.d_ls, a.d_la = (t.data_ptr() for t in g)
    a.image_l, a.image_u, a.label_l, a.perm_l, a.perm_u = (t.data_ptr() for t in keep)
    a.lam_l, a.lam_u = LAM_L, LAM_U
    a.B, a.D, a.K, a.bce, a.n_per_img, a.x_sigma = B, D, K, bce, npi, X_SIGMA
    a.sch = _sched(sch)
    a.terms, a.coef, a.tgt = terms.data_ptr(), coef.data_ptr(), tgt.data_ptr()
    L.call("sv_shot_loss_step", C.byref(a), st())
    torch.cuda.synchronize()
    got = {}
    for t, n, ids in ((g[0], "rec", (1, 3)), (g[1], "mu", (1, 3, 2, 4)), (g[2], "ls", (1, 3, 2, 4)), (g[3], "la", (1, 3, 2, 4))):
        for slot, i in enumerate(ids):
            got["%s%d" % (n, i)] = t[slot * B:(slot + 1) * B]
        tail_untouched(t, len(ids) * B, "d_" + n)
    _stage_check(terms[:12], coef[:10], tgt[:ntgt], r64[2], r32[2], got, r64, r32, "batched B=24")


def _compose_math(t, sch, dt):
    t = t.to(dt).requires_grad_(True)
    cp = sch["kl_beta_c"] * sch["pwm"]
    elbo_l = t[0] + sch["kl_beta_c"] * torch.abs(t[1] - sch["cmi"]) + sch["kl_beta_d"] * torch.abs(t[2] - sch["dmi"]) + cp * t[7]
    elbo_u = t[3] + sch["kl_beta_c"] * torch.abs(t[4] - sch["cmi"]) + sch["kl_beta_d"] * torch.abs(t[5] - sch["dmi"]) + cp * t[9]
    sup, unsup = sch["ew"] * elbo_l + t[6], sch["ew"] * elbo_u + sch["ucw"] * t[8]
    coef, = torch.autograd.grad(sup + unsup, t)                      # torch.abs has gradient 0 at 0
    return torch.stack([sup.detach(), unsup.detach()]), coef


@pytest.mark.parametrize("case", ["at_capacity", "across"])
def test_shot_compose_signs_at_and_around_the_capacities(case):
    """sign(0) = 0 (like torch.abs): a KL term exactly at its capacity gets the coefficient 0; one term on either side of each"""
    d = dev()
    sch = {k: f32v(v) for k, v in dict(ew=0.7, kl_beta_c=0.3, kl_beta_d=0.2, cmi=0.25, dmi=2.3, pwm=0.9, ucw=0.6).items()}
    cmi, dmi = sch["cmi"], sch["dmi"]
    if case == "at_capacity":       # klc_l == cmi, klc_u above; kld_l below, kld_u == dmi
        t = [3.0, cmi, dmi - 0.5, 2.5, cmi + 0.125, dmi, 1.1, 0.4, 0.9, 0.3]
    else:                           # klc_l below, klc_u above; kld_l above, kld_u below
        t = [3.0, cmi - 0.125, dmi + 0.5, 2.5, cmi + 1.0, dmi - 1.0, 1.1, 0.4, 0.9, 0.3]
    t = torch.tensor(t, dtype=F32)
    (s64, c64), (s32, c32) = _compose_math(t, sch, F64), _compose_math(t, sch, F32)
    terms, coef = buf(12), buf(10)
    terms[:10] = t.to(d)
    L.call("sv_shot_compose", p(terms), C.byref(_sched(sch)), p(coef), st())
    torch.cuda.synchronize()
    assert torch.equal(terms[:10].cpu(), t), "the ten input terms must be left as they were"
    close(terms[10:12], s32, s64, "compose losses " + case, each=True)
    nz = c64 != 0
    cf = coef[:10].cpu()
    close(cf[nz], c32[nz], c64[nz], "compose coef " + case, each=True)
    assert torch.equal(cf[~nz], torch.zeros(int((~nz).sum()))), "coefficient of a KL term AT its capacity must be 0"
    assert int((~nz).sum()) == (2 if case == "at_capacity" else 0)
    tail_untouched(terms, 12, "terms")
    tail_untouched(coef, 10, "coef")


@pytest.mark.parametrize("given", ["both", "sup_only", "unsup_only"])
def test_shot_scale_null_upstreams(given):
    d = dev()
    coef = torch.randn(10, generator=gen(41))
    gs, gu = torch.tensor([f32v(0.7)]), torch.tensor([f32v(-1.3)])
    up = torch.zeros(10, dtype=F64)
    sup = [0, 1, 2, 6, 7]                                             # the terms of loss_sup (steploss.TERMS)
    unsup = [3, 4, 5, 8, 9]
    if given != "unsup_only":
        up[sup] = gs.double()
    if given != "sup_only":
        up[unsup] = gu.double()
    gvec = buf(10)
    L.call("sv_shot_scale", p(coef.to(d)), p(gs.to(d)) if given != "unsup_only" else None,
           p(gu.to(d)) if given != "sup_only" else None, p(gvec), st())
    torch.cuda.synchronize()
    close(gvec[:10], coef * up.float(), coef.double() * up, "scale " + given)
    assert torch.equal(gvec[:10].cpu()[up == 0], torch.zeros(int((up == 0).sum()))), "a null upstream gradient is 0"
    tail_untouched(gvec, 10, "gvec")


@pytest.mark.parametrize("Bl,Bu", [(5, 5), (7, 3), (3, 7)])          # (5, 5): sv_shot_targets; Bl != Bu: sv_shot_targets2
@pytest.mark.parametrize("lam_dev", [0, 1])
def test_shot_targets_against_float64(lam_dev, Bl, Bu):
    D, K = 128, 10
    d = dev()
    g = gen(4200 + Bl)
    I = dict(mu1=torch.randn(Bl, D, generator=g), ls1=0.3 * torch.randn(Bl, D, generator=g), mu3=torch.randn(Bu, D, generator=g),
             ls3=0.3 * torch.randn(Bu, D, generator=g), la3=F.log_softmax(torch.randn(Bu, K, generator=g), dim=1))
    label, perm_l, perm_u = torch.randint(0, K, (Bl,), generator=g), torch.randperm(Bl, generator=g), torch.randperm(Bu, generator=g)
    T64 = _targets_math(*[I[k].double() for k in ("mu1", "ls1", "mu3", "ls3", "la3")], label, perm_l, perm_u, K, F64)
    T32 = _targets_math(*[I[k] for k in ("mu1", "ls1", "mu3", "ls3", "la3")], label, perm_l, perm_u, K, F32)
    out = {k: buf(*T64[k].shape) for k in ("sm_mu", "sm_sigma", "lab_mix", "mx_mu", "mx_sigma", "mx_alpha")}
    lams = torch.tensor([LAM_L, LAM_U], device=d)
    lam = (-3.0, C.c_void_p(lams.data_ptr()), 5.0, C.c_void_p(lams.data_ptr() + 4)) if lam_dev else (LAM_L, None, LAM_U, None)
    ins = [p(I[k].to(d)) for k in ("mu1", "ls1", "mu3", "ls3", "la3")] + [p(label.to(d)), p(perm_l.to(d)), p(perm_u.to(d))]
    outs = [p(out[k]) for k in ("sm_mu", "sm_sigma", "lab_mix", "mx_mu", "mx_sigma", "mx_alpha")]
    if Bl == Bu:
        L.call("sv_shot_targets", *ins, *lam, Bl, D, K, *outs, st())
    else:
        L.call("sv_shot_targets2", *ins, *lam, Bl, Bu, D, K, *outs, st())
    torch.cuda.synchronize()
    for k in out:
        n = T64[k].shape[0]
        close(out[k][:n], T32[k], T64[k], "targets %s Bl=%d Bu=%d" % (k, Bl, Bu))
        tail_untouched(out[k], n, "targets " + k)


# ------------------------------------------------------------------------------------------------ 5. pairing and mixing
# (B, D): the smallest batch | the argmin loop's second trip (B > 64) and its cross-lane tie rule | the j += 256 loop's second trip
# (the workload's B is 512) | the same with D = 100 | D = 512: the staging loop d += 256 takes two trips
MATCH_SHAPES = [(2, 128), (70, 128), (300, 128), (300, 100), (130, 512)]


def _match_inputs(B, D, seed):
    g = gen(seed)
    return torch.randn(B, D, generator=g), 0.3 * torch.randn(B, D, generator=g)


def _match_run(mu, ls):
    B, D = mu.shape
    got = torch.full((B + GUARD,), -1, dtype=torch.int64, device=dev())
    L.call("sv_optimal_match", p(mu.to(dev())), p(ls.to(dev())), B, D, p(got), st())
    torch.cuda.synchronize()
    assert torch.equal(got[B:].cpu(), torch.full((GUARD,), -1, dtype=torch.int64)), "index: guard tail written"
    return got[:B].cpu()


@pytest.mark.parametrize("B,D", MATCH_SHAPES)
def test_optimal_match_against_float64(B, D):
    """the index must be the float64 second-smallest of each row of pairwise_gaussian_kl wherever that row's float64 gaps (first
    to second, second to third) exceed margin = 20 x the largest error of the fp32 restatement of the KL matrix; at most 2 % of
    the rows may be left out that way (a condition on the test's data, not a tolerance)"""
    mu, ls = _match_inputs(B, D, 1)
    kl64 = O.pairwise_gaussian_kl(mu.double(), ls.double())
    kl32 = O.pairwise_gaussian_kl(mu, ls)
    margin = 20.0 * float((kl32.double() - kl64).abs().max())
    srt, idx = torch.sort(kl64, dim=1)
    gap = srt[:, 1] - srt[:, 0]
    if B > 2:
        gap = torch.minimum(gap, srt[:, 2] - srt[:, 1])
    decided = gap > margin
    print("FIG %-34s margin %.3e KL %.3g..%.3g undecided rows %d" % ("match B=%d D=%d" % (B, D), margin, float(srt[:, 1].min()),
                                                                     float(srt[:, 1].max()), int((~decided).sum())))
    assert int((~decided).sum()) <= 0.02 * B, "test data: too many rows with a float64 gap below the margin"
    got = _match_run(mu, ls)
    assert ((got >= 0) & (got < B)).all()
    assert torch.equal(got[decided], idx[:, 1][decided]), "rows %s" % torch.nonzero(got != idx[:, 1]).view(-1).tolist()


def test_optimal_match_tie_rule_lower_index_first():
    """rows 3 and 68 bit-identical: KL(3 || 3) and KL(3 || 68) are the same bits, so the first pass takes the lower index 3 and
    the second pass 68 -- for row 3 and for row 68 alike"""
    mu, ls = _match_inputs(70, 128, 2)
    mu[3], ls[3] = mu[68], ls[68]
    got = _match_run(mu, ls)
    assert int(got[3]) == 68 and int(got[68]) == 68, (int(got[3]), int(got[68]))


def test_optimal_match_refuses_what_does_not_fit_lds():
    """2 D + B floats beyond 64 KB: SV_E_SHAPE as an error code, no launch"""
    B, D = 2, 8192
    d = dev()
    mu, ls = torch.zeros(B, D, device=d), torch.zeros(B, D, device=d)
    got = torch.full((B,), -1, dtype=torch.int64, device=d)
    assert (2 * D + B) * 4 > 64 * 1024
    rc = L.lib().sv_optimal_match(p(mu), p(ls), B, D, p(got), st())
    torch.cuda.synchronize()
    assert rc == SV_E_SHAPE, rc
    assert b"sv_optimal_match" in L.lib().sv_last_error()
    assert torch.equal(got.cpu(), torch.full((B,), -1, dtype=torch.int64))


@pytest.mark.parametrize("row", [1, 255, 257, 3072])
@pytest.mark.parametrize("exp_space", [0, 1])
@pytest.mark.parametrize("lam_dev", [0, 1])
def test_mix_lerp_against_float64(lam_dev, exp_space, row):
    """mix_with_index: lam * a + (1 - lam) * a[index], sigma / alpha in linear space (exp_space)"""
    B = 9
    d = dev()
    a = 0.5 * torch.randn(B, row, generator=gen(5000 + row))
    index = torch.tensor([0, 2, 1, 3, 5, 4, 8, 7, 6])                          # a permutation with fixed points (0, 3, 7)
    f = (lambda t: torch.exp(t)) if exp_space else (lambda t: t)
    mix = lambda t: LAM * f(t) + (1 - LAM) * f(t)[index]
    out = buf(B, row)
    lam_t = torch.tensor([LAM], device=d) if lam_dev else None
    L.call("sv_mix_lerp", p(a.to(d)), p(index.to(d)), -7.0 if lam_dev else LAM, p(lam_t), B, row, exp_space, p(out), st())
    torch.cuda.synchronize()
    close(out[:B], mix(a), mix(a.double()), "mix_lerp row=%d exp=%d" % (row, exp_space))
    tail_untouched(out, B, "mix_lerp out")


@pytest.mark.parametrize("B,row", [(0, 64), (9, 0)])
def test_mix_lerp_empty_is_ok_without_a_launch(B, row):
    d = dev()
    a, index, out = torch.zeros(16, device=d), torch.zeros(9, dtype=torch.int64, device=d), buf(16)
    L.call("sv_mix_lerp", p(a), p(index), LAM, None, B, row, 0, p(out), st())
    torch.cuda.synchronize()
    tail_untouched(out, 0, "mix_lerp out")


# ------------------------------------------------------------------------------------------------ 6. optimizers
# n: below one vector | tail 3 | no tail, several blocks | tail 1; sv_adam: past its 2 048-block cap (the grid-stride loop)
OPT_N = [3, 1003, 4096, 600001]
STEPS = 5


def _special_grads(n, g, step):
    """gradients of 0, 1e-20 (sqrt(v) << eps) and 1e4 in front of N(0, 1) ones"""
    x = torch.randn(n, generator=g)
    x[:3] = torch.tensor([0.0, 1e-20, 1e4])[:n] * (1.0 if step % 2 == 0 else -1.0)
    return x


def _opt_check(name, dev_bufs, s32, s64, w, n, tag):
    """the parameters as the accumulated update p - p0 (an error of 1e-3 of an Adam update is 1e-6 of p itself); Adam's state
    buffers in two groups (the 1e4 gradient would hide every other element's error)"""
    for k, t in dev_bufs.items():
        what = "%s %s %s" % (name, k, tag)
        tail_untouched(t, n, what)
        if k == "p":
            close(t[:n].cpu().double() - w.double(), s32[k].double() - w.double(), s64[k] - w.double(), what + " - p0")
        elif name == "sgd":
            close(t[:n], s32[k], s64[k], what)
        else:
            close(t[:3], s32[k][:3], s64[k][:3], what + " special")
            if n > 3:
                close(t[3:n], s32[k][3:], s64[k][3:], what + " ordinary")


@pytest.mark.parametrize("n", OPT_N)
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_sgd_against_float64_torch_sgd(wd, n):
    d = dev()
    g = gen(6000 + n)
    w = torch.randn(n, generator=g)
    lr, mom, wdf, gscale = f32v(0.1), f32v(0.9), f32v(wd), 0.25
    prm = {dt: torch.nn.Parameter(w.to(dt).clone()) for dt in (F64, F32)}
    opt = {dt: torch.optim.SGD([prm[dt]], lr=lr, momentum=mom, weight_decay=wdf) for dt in prm}
    bufs = dict(p=filled(w), v=buf(n))                                       # (the first step overwrites v)
    for step in range(STEPS):
        graw = 4.0 * torch.randn(n, generator=g)
        state = {}
        for dt in prm:
            prm[dt].grad = graw.to(dt) * gscale
            opt[dt].step()
            state[dt] = dict(p=prm[dt].detach(), v=opt[dt].state[prm[dt]]["momentum_buffer"])
        L.call("sv_sgd", p(bufs["p"]), p(graw.to(d)), p(bufs["v"]), n, lr, mom, wdf, gscale, int(step == 0), st())
        torch.cuda.synchronize()
        _opt_check("sgd", bufs, state[F32], state[F64], w, n, "n=%d wd=%g step %d" % (n, wd, step + 1))


@pytest.mark.parametrize("n", OPT_N)
def test_adam_against_float64_torch_adam(n):
    """five steps with the step count by value, then five through step_dev with the by-value count poisoned"""
    d = dev()
    g = gen(6100 + n)
    w = torch.randn(n, generator=g)
    lr, b1, b2, eps, gscale = f32v(1e-3), f32v(0.9), f32v(0.999), f32v(1e-8), 0.5
    prm = {dt: torch.nn.Parameter(w.to(dt).clone()) for dt in (F64, F32)}
    opt = {dt: torch.optim.Adam([prm[dt]], lr=lr, betas=(b1, b2), eps=eps) for dt in prm}
    bufs = dict(p=filled(w), m=filled(torch.zeros(n)), v=filled(torch.zeros(n)))
    step_dev = torch.zeros(1, device=d)
    for step in range(1, 2 * STEPS + 1):
        graw = _special_grads(n, g, step)
        state = {}
        for dt in prm:
            prm[dt].grad = graw.to(dt) * gscale
            opt[dt].step()
            s = opt[dt].state[prm[dt]]
            state[dt] = dict(p=prm[dt].detach(), m=s["exp_avg"], v=s["exp_avg_sq"])
        by_dev = step > STEPS
        step_dev.fill_(float(step))
        L.call("sv_adam", p(bufs["p"]), p(graw.to(d)), p(bufs["m"]), p(bufs["v"]), n, lr, b1, b2, eps, 1000.0 if by_dev else float(step),
               p(step_dev) if by_dev else None, gscale, st())
        torch.cuda.synchronize()
        _opt_check("adam", bufs, state[F32], state[F64], w, n, "n=%d step %d%s" % (n, step, " dev" if by_dev else ""))
