"""PreActResNet-18 / 34 encoders on a real MI355X: the 4 x 4-map instantiations of the stride-1 3x3 kernels through sv_igemm /
sv_wgrad against plain torch fp32 (wgrad3x3.hip: on by default, SV_K_MAP4 in the disable mask switches it off; conv3x3.hip forward /
data gradient: measured no faster than the gather-GEMM, off by default, SV_K_MAP4_CONV in the enable mask switches it on), and the model against the
reference's own outputs (tests/golden/ref_*_preact*.npz) and the CPU oracle (tests/_preact_oracle.py).

Tolerances are the project's: kernels 2e-4 of tensor scale in fp32-operand mode, 2.5e-2 in bf16; the step
1e-3 in fp32-operand mode, bf16 losses 5e-3 and tensors 3e-2 of max-abs."""
import ctypes as C_

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                     # noqa: E402
from shot_vae_amd import _lib as L           # noqa: E402
from shot_vae_amd import geometry as G       # noqa: E402
from oracle import closed_form as C          # noqa: E402
from oracle import shotvae_oracle as O       # noqa: E402
from tests import _cases as T                # noqa: E402
from tests import _preact_oracle as P        # noqa: E402
oracle_step, PREACT_STEP = P.oracle_step, P.PREACT_STEP

DT = {"f32": (L.SV_F32, torch.float32, 2e-4), "bf16": (L.SV_BF16, torch.bfloat16, 2.5e-2)}
FP32_TOL = 1e-3


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def st():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def bq(t, dt):
    return t.to(DT[dt][1]).float()


def repack(master, g, transpose, dt):
    code, tdt, _ = DT[dt]
    N, Tt, Cc = master.shape
    dst = torch.zeros(max(G.packed_size(g), 1), dtype=tdt, device=dev())
    m = master.to(dev()).contiguous()
    L.call("sv_repack", code, C_.c_void_p(m.data_ptr()), N, Tt, Cc, int(transpose), C_.byref(g), C_.c_void_p(dst.data_ptr()), st())
    torch.cuda.synchronize()
    return dst


def igemm(g, dt, x, w, Gn=1, pro=None, residual=None, stats=False, ex=None, enable=L.K_MAP4_CONV):
    """sv_igemm on Gn groups of g.B images; pro = (scale [Gn][C], shift [Gn][C], slope); returns (out, sums [Gn][2N] or None, grid)"""
    code, tdt, _ = DT[dt]
    d = dev()
    keep = []

    def on(t, ty=torch.float32):
        t = t.to(d, ty).contiguous()
        keep.append(t)
        return t.data_ptr()

    out = torch.full((Gn * g.B, g.Hout, g.Wout, g.ldo), 7.0, dtype=tdt, device=d)
    a = L.SvIgemmArgs()
    a.x, a.w, a.out, a.groups = on(x, tdt), w.data_ptr(), out.data_ptr(), Gn
    if pro is not None:
        a.pro_scale, a.pro_shift, a.pro_slope = on(pro[0]), on(pro[1]), pro[2]
    if residual is not None:
        a.residual = on(residual, tdt)
    a.replicas = 1
    sums = None
    with L.options(enable=enable):
        if ex is not None:
            a.ex = on(ex["x"], tdt)
            a.ex_scale, a.ex_shift, a.ex_mean, a.ex_rstd = [on(ex[k]) for k in ("scale", "shift", "mean", "rstd")]
            a.ex_slope = ex["slope"]
        if stats or ex is not None:
            a.stats = a.x              # (placeholder for the grid query)
            if ex is not None:
                a.stats, a.bsums = None, a.x
            R = L.det_replicas(g, code, a) if L.det_stats() else 4
            sums = torch.zeros(Gn, R, 2 * g.N, device=d, dtype=torch.float64)
            a.replicas = R
            if ex is not None:
                a.bsums = sums.data_ptr()
            else:
                a.stats = sums.data_ptr()
        blocks = C_.c_int(0)
        L.call("sv_igemm_query_blocks", C_.byref(g), code, C_.byref(a), C_.byref(blocks))
        L.call("sv_igemm", C_.byref(g), code, C_.byref(a), st())
        torch.cuda.synchronize()
    return out.float().cpu(), (None if sums is None else sums.sum(1).float().cpu()), blocks.value


def map4_grid(B, N, dt):
    """blocks in x of the 4 x 4-map instantiation: (B / 8 tiles of eight whole images) x (channel tiles of 64, or 32)"""
    bn = 64 if (dt == "bf16" and N % 64 == 0) else 32
    return (B // 8) * (N // bn)


def took_map4(grids, outs, want, decisive):
    """The enabled launch took the 4 x 4 instantiation: sv_igemm_query_blocks reports ITS grid for the launch -- (B / 8) tiles x
    channel tiles.  On the shape that matters (512 -> 512, `decisive`) the run with the mask set must be visibly another kernel:
    another grid, or -- where the two grids coincide (fp32 at 16 images: 2 x 16 either way) -- other bits, since the two kernels
    add the 9 * Cin products in different orders.  For the small shapes the general path can have the same grid AND, after the
    rounding to bf16, the same bits (96 -> 160 at 8 images: 5 blocks, identical outputs): nothing the library reports tells the two
    apart there, so only the grid is held."""
    assert grids[0] == want, (grids, want)
    if decisive:
        assert grids[1] != grids[0] or not torch.equal(outs[0], outs[1]), grids


def act(u, slope):
    return torch.where(u > 0, u, u * slope)


# B, Cin, N, groups
MAP4_CASES = [(16, 512, 512, 1), (8, 96, 160, 1), (8, 96, 160, 4), (24, 64, 96, 1), (8, 512, 512, 4)]


# ------------------------------------------------------------------------------------------------------- construction
def test_preactresnet18_constructs_and_runs_forward():
    """THE feature: on the parent commit this raises NotImplementedError in the constructor."""
    m = S.VariationalAutoEncoder("preactresnet18", 3, 0, (32, 32), data_parallel=True, continuous_latent_dim=128, disc_latent_dim=10,
                                 small_input=True).cuda().train()
    x = torch.rand(8, 3, 32, 32, device="cuda")
    rec, mu, ls, la = m(x)
    torch.cuda.synchronize()
    assert rec.shape == (8, 3, 32, 32) and mu.shape == (8, 128) and ls.shape == (8, 128) and la.shape == (8, 10)
    assert all(bool(torch.isfinite(t).all()) for t in (rec, mu, ls, la))
    assert abs(float(torch.exp(la.detach()).sum(1).mean()) - 1.0) < 1e-4
    (rec.sum() + mu.sum() + la[:, 0].sum()).backward()
    torch.cuda.synchronize()
    k = "feature_extractor.encoder.block4.module.preact_block.unit2.f_block.conv2.weight"
    gr = dict(m.named_parameters())[k].grad
    assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------------- kernels
# (deterministic mode -- SV_OPT_DETERMINISTIC = 1 -- at slope 0 on the one-group shapes)
FWD_CASES = [(c, s, 0) for c in MAP4_CASES for s in (0.0, 0.01, 1.0)] + [(c, 0.0, 1) for c in MAP4_CASES if c[3] == 1]
WGRAD_CASES = [(c, w, 0) for c in MAP4_CASES for w in (True, False)] + [(c, True, 1) for c in MAP4_CASES]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case,slope,det", FWD_CASES)
def test_map4_forward(case, dt, slope, det):
    """forward of a stride-1 3x3 layer on 4 x 4 maps: BatchNorm + activation prologue (per group), residual, statistics; the new
    instantiation (asserted through the grid sv_igemm reports for the launch) and, switched off, the parent's path"""
    B, Cin, N, Gn = case
    tol = DT[dt][2]
    torch.manual_seed(B + Cin + Gn)
    x = bq(torch.randn(Gn * B, Cin, 4, 4), dt)
    w = bq(torch.randn(N, Cin, 3, 3) / (Cin * 9) ** 0.5, dt)
    scale, shift = torch.rand(Gn, Cin) + 0.5, torch.randn(Gn, Cin) * 0.3
    res = bq(torch.randn(Gn * B, N, 4, 4), dt)
    sg, hg = scale.repeat_interleave(B, 0)[:, :, None, None], shift.repeat_interleave(B, 0)[:, :, None, None]
    y = F.conv2d(bq(act(x * sg + hg, slope), dt), w, None, 1, 1) + res
    g = G.conv_like(B, 4, 4, Cin, N, 3, 1, 1)
    wp = repack(w.permute(0, 2, 3, 1).reshape(N, 9, Cin).contiguous(), g, False, dt)
    grids, outs = [], []
    with L.options(deterministic=det):
        for mask in (L.K_MAP4_CONV, 0):
            out, sums, grid = igemm(g, dt, nhwc(x), wp, Gn, pro=(scale, shift, slope), residual=nhwc(res), stats=True, enable=mask)
            grids.append(grid)
            outs.append(out)
            e = rel(nchw(out), y)
            print("map4 fwd", case, dt, slope, "mask", mask, "grid", grid, "err %.3e" % e)
            assert e < tol, (mask, e)
            yg = y.view(Gn, B, N, 4, 4)
            assert rel(sums[:, :N], yg.sum((1, 3, 4))) < max(tol, 1e-3) * 3
            assert rel(sums[:, N:], (yg * yg).sum((1, 3, 4))) < max(tol, 1e-3) * 3
    took_map4(grids, outs, map4_grid(B, N, dt), (Cin, N, Gn) == (512, 512, 1))


@pytest.mark.parametrize("slope", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", MAP4_CASES)
def test_map4_dgrad(case, dt, slope):
    """data gradient with the activation-backward epilogue (g = dL/da * act'(BN(x)), sums of g and g * xhat per group)"""
    B, Cin, N, Gn = case
    tol = DT[dt][2]
    torch.manual_seed(B + N)
    w = bq(torch.randn(N, Cin, 3, 3) / (Cin * 9) ** 0.5, dt)
    dy = bq(torch.randn(Gn * B, N, 4, 4), dt)
    xraw = bq(torch.randn(Gn * B, Cin, 4, 4), dt)
    scale, shift = torch.rand(Gn, Cin) + 0.5, torch.randn(Gn, Cin) * 0.3
    mean, rstd = torch.randn(Gn, Cin) * 0.1, torch.rand(Gn, Cin) + 0.5
    ri = lambda v: v.repeat_interleave(B, 0)[:, :, None, None]          # noqa: E731
    da = F.conv_transpose2d(dy, w, None, 1, 1)
    u = xraw * ri(scale) + ri(shift)
    gref = da * torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))
    xh = (xraw - ri(mean)) * ri(rstd)
    g = G.convT_like(B, 4, 4, N, Cin, 3, 1, 1)
    wp = repack(w.permute(0, 2, 3, 1).reshape(N, 9, Cin).contiguous(), g, True, dt)
    grids, outs = [], []
    for mask in (L.K_MAP4_CONV, 0):
        out, sums, grid = igemm(g, dt, nhwc(dy), wp, Gn, ex=dict(x=nhwc(xraw), scale=scale, shift=shift, mean=mean, rstd=rstd, slope=slope),
                                enable=mask)
        grids.append(grid)
        outs.append(out)
        e = rel(nchw(out), gref)
        print("map4 dgrad", case, dt, slope, "mask", mask, "grid", grid, "err %.3e" % e)
        assert e < tol, (mask, e)
        gg, xg = gref.view(Gn, B, Cin, 4, 4), xh.view(Gn, B, Cin, 4, 4)
        assert rel(sums[:, :Cin], gg.sum((1, 3, 4))) < max(tol, 1e-3) * 3
        assert rel(sums[:, Cin:], (gg * xg).sum((1, 3, 4))) < max(tol, 1e-3) * 3
    took_map4(grids, outs, map4_grid(B, Cin, dt), (Cin, N, Gn) == (512, 512, 1))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case,use_ws,det", WGRAD_CASES)
def test_map4_wgrad(case, dt, use_ws, det):
    """weight gradient on 4 x 4 maps (prologue slope 0 = ReLU, groups with their own coefficients, accumulation into a non-zero
    gradient, with and without the partial-slab workspace), default dispatch and SV_K_MAP4 off, and -- in deterministic mode --
    the assertion that the default run is another kernel than the general one."""
    B, Cin, N, Gn = case
    code, tdt, tol = DT[dt]
    torch.manual_seed(B + Cin)
    d = dev()
    x = bq(torch.randn(Gn * B, Cin, 4, 4), dt)
    dy = bq(torch.randn(Gn * B, N, 4, 4), dt)
    scale, shift = torch.rand(Gn, Cin) + 0.5, torch.randn(Gn, Cin) * 0.3
    ri = lambda v: v.repeat_interleave(B, 0)[:, :, None, None]          # noqa: E731
    a_in = bq(act(x * ri(scale) + ri(shift), 0.0), dt)
    wref = torch.nn.grad.conv2d_weight(a_in, (N, Cin, 3, 3), dy, 1, 1)
    g = G.conv_like(B, 4, 4, Cin, N, 3, 1, 1)
    xd, dyd = nhwc(x).to(d, tdt).contiguous(), nhwc(dy).to(d, tdt).contiguous()
    sc, sh = scale.to(d).contiguous(), shift.to(d).contiguous()
    ws = torch.full((16 * 1024 * 1024,), float("nan"), device=d) if use_ws else None

    def run(mask):
        dw = torch.full((N, 9, Cin), 0.5, device=d)
        a = L.SvWgradArgs()
        a.x, a.dy, a.dw = xd.data_ptr(), dyd.data_ptr(), dw.data_ptr()
        a.pro_scale, a.pro_shift, a.pro_slope = sc.data_ptr(), sh.data_ptr(), 0.0
        a.splits, a.use_tr, a.groups, a.block_budget = 0, 1, Gn, 0
        if use_ws:
            a.ws, a.ws_elems = ws.data_ptr(), ws.numel()
        with L.options(disable=mask, deterministic=det):
            L.call("sv_wgrad_ex", C_.byref(g), code, C_.byref(a), st())
            torch.cuda.synchronize()
        return (dw.cpu() - 0.5).view(N, 3, 3, Cin).permute(0, 3, 1, 2)

    got, ref = run(0), run(L.K_MAP4)
    e0, e1 = rel(got, wref), rel(ref, wref)
    print("map4 wgrad", case, dt, "ws", use_ws, "det", det, "err %.3e (off: %.3e)" % (e0, e1))
    assert e0 < max(tol, 2e-3 if dt == "bf16" else tol) and e1 < max(tol, 2e-3 if dt == "bf16" else tol)
    if det:
        # fixed summation order: each path reproduces itself bit for bit, so bits that differ BETWEEN the two masks can only come
        # from another kernel -- the default run took the 4 x 4 instantiation, SV_K_MAP4 switched it off.  (The library reports no
        # kernel identity for sv_wgrad; test_map4_partial_tile_stays_general holds the converse: where the instantiation must
        # refuse, the mask changes nothing.)
        assert torch.equal(got, run(0)), "deterministic mode: two runs of the 4 x 4 weight gradient differ"
        assert torch.equal(ref, run(L.K_MAP4)), "deterministic mode: two runs of the general weight gradient differ"
        assert not torch.equal(got, ref), "SV_K_MAP4 did not change the weight-gradient kernel"


@pytest.mark.parametrize("B", [5, 12])
def test_map4_partial_tile_stays_general(B):
    """B * 4 rows is not a multiple of the 32-row tile: the *_try functions leave the layer to the general path -- forward and data
    gradient (same grid and bits with the instantiation enabled and not) and the weight gradient (deterministic mode: same bits
    with SV_K_MAP4 on and off) -- with results as before"""
    dt, Cin, N = "bf16", 64, 96
    tol = DT[dt][2]
    torch.manual_seed(B)
    x = bq(torch.randn(B, Cin, 4, 4), dt)
    w = bq(torch.randn(N, Cin, 3, 3) / (Cin * 9) ** 0.5, dt)
    dy = bq(torch.randn(B, N, 4, 4), dt)
    master = w.permute(0, 2, 3, 1).reshape(N, 9, Cin).contiguous()
    g = G.conv_like(B, 4, 4, Cin, N, 3, 1, 1)
    wp = repack(master, g, False, dt)
    o0, _, g0 = igemm(g, dt, nhwc(x), wp)
    o1, _, g1 = igemm(g, dt, nhwc(x), wp, enable=0)
    assert g0 == g1 and rel(nchw(o0), F.conv2d(x, w, None, 1, 1)) < tol and torch.equal(o0, o1)
    gd = G.convT_like(B, 4, 4, N, Cin, 3, 1, 1)
    wpd = repack(master, gd, True, dt)
    o0, _, g0 = igemm(gd, dt, nhwc(dy), wpd)
    o1, _, g1 = igemm(gd, dt, nhwc(dy), wpd, enable=0)
    assert g0 == g1 and rel(nchw(o0), F.conv_transpose2d(dy, w, None, 1, 1)) < tol and torch.equal(o0, o1)
    d = dev()
    xd, dyd = nhwc(x).to(d, torch.bfloat16).contiguous(), nhwc(dy).to(d, torch.bfloat16).contiguous()
    ws = torch.empty(4 * 1024 * 1024, device=d)
    res = []
    for mask in (0, L.K_MAP4):
        dw = torch.zeros(N, 9, Cin, device=d)
        a = L.SvWgradArgs()
        a.x, a.dy, a.dw = xd.data_ptr(), dyd.data_ptr(), dw.data_ptr()
        a.splits, a.use_tr, a.groups, a.block_budget, a.ws, a.ws_elems = 0, 1, 1, 0, ws.data_ptr(), ws.numel()
        with L.options(disable=mask, deterministic=1):
            L.call("sv_wgrad_ex", C_.byref(g), L.SV_BF16, C_.byref(a), st())
            torch.cuda.synchronize()
        res.append(dw.cpu().view(N, 3, 3, Cin).permute(0, 3, 1, 2))
    assert rel(res[0], torch.nn.grad.conv2d_weight(x, (N, Cin, 3, 3), dy, 1, 1)) < 2e-3
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_map4_images_are_isolated(dt):
    """Eight whole images share a tile, their rows back to back in the staged halo: give every image a different constant and
    all-ones weights -- an output pixel is then (number of in-bounds taps) * Cin * its OWN image's constant, exactly (small
    integers), in the forward, the data gradient and the weight gradient.  One neighbour row leaking in would change it."""
    code, tdt, _ = DT[dt]
    B, Cc = 16, 32
    const = torch.arange(1, B + 1, dtype=torch.float32)
    x = const[:, None, None, None].expand(B, Cc, 4, 4).contiguous()
    w = torch.ones(Cc, Cc, 3, 3)
    cnt = F.conv2d(torch.ones(1, 1, 4, 4), torch.ones(1, 1, 3, 3), None, 1, 1)[0, 0]        # 4 / 6 / 9 taps in bounds
    want = (const[:, None, None, None] * cnt[None, None] * Cc).expand(B, Cc, 4, 4)
    for transpose, g in ((False, G.conv_like(B, 4, 4, Cc, Cc, 3, 1, 1)), (True, G.convT_like(B, 4, 4, Cc, Cc, 3, 1, 1))):
        wp = repack(w.permute(0, 2, 3, 1).reshape(Cc, 9, Cc).contiguous(), g, transpose, dt)
        out, _, grid = igemm(g, dt, nhwc(x), wp)
        assert grid == map4_grid(B, Cc, dt)
        assert torch.equal(nchw(out), want), (transpose, (nchw(out) - want).abs().max())
    # weight gradient: dy = 1 on image b only -> dW[n][tap][c] = b's constant * (pixels whose tap is in bounds)
    d = dev()
    g = G.conv_like(B, 4, 4, Cc, Cc, 3, 1, 1)
    for b in (0, 7, 8, 15):
        dy = torch.zeros(B, Cc, 4, 4)
        dy[b] = 1.0
        dw = torch.zeros(Cc, 9, Cc, device=d)
        xd, dyd = nhwc(x).to(d, tdt).contiguous(), nhwc(dy).to(d, tdt).contiguous()
        L.call("sv_wgrad", C_.byref(g), code, C_.c_void_p(xd.data_ptr()), None, None, 0.0, C_.c_void_p(dyd.data_ptr()),
               C_.c_void_p(dw.data_ptr()), 0, 1, None, 0, 1, st())
        torch.cuda.synchronize()
        ref = torch.nn.grad.conv2d_weight(x, (Cc, Cc, 3, 3), dy, 1, 1)
        assert torch.equal(dw.cpu().view(Cc, 3, 3, Cc).permute(0, 3, 1, 2), ref), b


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_shortcut_with_slope_one(dt):
    """the PreActResNet shortcut: BatchNorm WITHOUT an activation (slope 1) in front of a 1x1 stride-2 convolution, forward and
    the data gradient's activation-backward epilogue (act' = 1 everywhere), against torch autograd"""
    B, Cin, N, H = 8, 64, 128, 32
    tol = DT[dt][2]
    torch.manual_seed(3)
    x = bq(torch.randn(B, Cin, H, H), dt).requires_grad_(True)
    w = bq(torch.randn(N, Cin, 1, 1) / Cin ** 0.5, dt)
    scale, shift = torch.rand(1, Cin) + 0.5, torch.randn(1, Cin) * 0.3
    a = x * scale[0][None, :, None, None] + shift[0][None, :, None, None]
    aq = a + (bq(a.detach(), dt) - a.detach())           # the operand rounding, straight-through
    y = F.conv2d(aq, w, None, 2, 0)
    dy = bq(torch.randn_like(y), dt)
    y.backward(dy)
    gref = x.grad / scale[0][None, :, None, None]         # dL/d(BN output): the epilogue's result (sv_bn_bwd_apply does the rest)
    g = G.conv_like(B, H, H, Cin, N, 1, 2, 0)
    wp = repack(w.permute(0, 2, 3, 1).reshape(N, 1, Cin).contiguous(), g, False, dt)
    out, _, _ = igemm(g, dt, nhwc(x.detach()), wp, pro=(scale, shift, 1.0))
    assert rel(nchw(out), y.detach()) < tol
    gd = G.convT_like(B, H // 2, H // 2, N, Cin, 1, 2, 0)
    wpd = repack(w.permute(0, 2, 3, 1).reshape(N, 1, Cin).contiguous(), gd, True, dt)
    mean, rstd = torch.randn(1, Cin) * 0.1, torch.rand(1, Cin) + 0.5
    out, sums, _ = igemm(gd, dt, nhwc(dy), wpd, ex=dict(x=nhwc(x.detach()), scale=scale, shift=shift, mean=mean, rstd=rstd, slope=1.0))
    assert rel(nchw(out), gref) < tol
    assert rel(sums[0, :Cin], gref.sum((0, 2, 3))) < max(tol, 1e-3) * 3


# ------------------------------------------------------------------------------------------------------- the model
def make_model(name, dtype, state=None, dp=False, K=10, **kw):
    m = S.VariationalAutoEncoder(encoder_name=name, num_input_channels=3, drop_rate=kw.pop("drop_rate", 0), img_size=(32, 32),
                                 data_parallel=dp, continuous_latent_dim=128, disc_latent_dim=K, sample_temperature=0.67,
                                 small_input=True, compute_dtype=dtype, **kw)
    if state is not None:
        m.load_state_dict({k: v.detach() for k, v in state.items()})
    return m.cuda().train()


def param_grads(model):
    return {k.replace(".module.", "."): p.grad.detach().float().cpu().clone() for k, p in model.named_parameters()}


def _state(name, K=10):
    with P.patched():
        return C.make_state(name, K=K)


@pytest.mark.parametrize("grouped", [False, True])
def test_step_matches_reference_golden_fp32(grouped):
    """the reference's own step on preactresnet18 (B_l = B_u = 8: the 4 x 4 layers take the new kernels), sequential and grouped,
    held as tests/test_model_gpu.py holds the WideResNet fixtures"""
    name, K, Bl, Bu = PREACT_STEP
    g = T.load("ref_step_preact18_br")
    model = make_model(name, "fp32", _state(name))
    elbo, cls = S.VAECriterion(discrete_dim=K, x_sigma=1.0, bce_reconstruction=True).cuda(), S.ClsCriterion()
    opt = S.FlatSGD(model, lr=0.1, momentum=0.9, weight_decay=5e-4)
    opt.zero_grad()
    sch = O.schedule(10)
    names = [str(n) for n in g["meta.param_names"]]
    il, ll, iu, lu = C.make_batch(Bl, Bu, K, stream0=7000)
    nz = C.make_noise(Bl, Bu, K, stream0=9000)
    step = S.train_step_grouped if grouped else S.train_step
    with T.rng_for_step(nz):
        out = step(model, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), sch, return_outputs=True)
    torch.cuda.synchronize()
    for k in T.SCALARS:
        ref = float(g["s0." + k])
        print(k, float(out[k]), ref)
        assert abs(float(out[k]) - ref) <= FP32_TOL * max(abs(ref), 1e-6), (k, float(out[k]), ref)
    for k in T.TENSORS:
        if k not in out:          # (the grouped step does not compute the unused reconstructions rec2 / rec4)
            assert grouped and k in ("rec2", "rec4")
            continue
        e = T.rel_err(out[k].float().cpu().numpy(), g["s0." + k])
        print(k, "%.3e" % e)
        assert e < FP32_TOL, (k, e)
    grads = param_grads(model)
    gn = np.array([float(grads[k].double().norm()) for k in names])
    gr = g["s0.grad_norm"]
    bad = np.abs(gn - gr) > 1e-2 * gr + 1e-4 * gr.max()
    assert not bad.any(), [(names[i], gn[i], gr[i]) for i in np.nonzero(bad)[0][:5]]
    gs = np.concatenate([grads[k].reshape(-1)[torch.from_numpy(T.sample_idx(grads[k].numel()))].numpy() for k in names])
    e_gs = T.rel_err(gs, g["s0.grad_sample"])
    print("grad_sample %.3e" % e_gs)
    assert e_gs < 1e-2
    opt.step()
    torch.cuda.synchronize()
    sd = {k.replace(".module.", "."): v.detach().float().cpu() for k, v in model.state_dict().items()}
    pn = np.array([float(sd[k].double().norm()) for k in names])
    assert np.max(np.abs(pn - g["final.param_norm"]) / g["final.param_norm"]) < 1e-3
    ps = np.concatenate([sd[k].reshape(-1)[torch.from_numpy(T.sample_idx(sd[k].numel()))].numpy() for k in names])
    assert T.rel_err(ps, g["final.param_sample"]) < 1e-3
    for k in g.files:
        if k.startswith("final.buf."):
            assert T.rel_err(sd[k[len("final.buf."):]].numpy(), g[k]) < 1e-3, k


def test_step_bf16_against_reference_golden():
    """bf16 operands at the project's gates: losses 5e-3, tensors 3e-2 of max-abs (measured values are printed)"""
    name, K, Bl, Bu = PREACT_STEP
    g = T.load("ref_step_preact18_br")
    model = make_model(name, "bf16", _state(name), dp=True)
    elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
    il, ll, iu, lu = C.make_batch(Bl, Bu, K, stream0=7000)
    nz = C.make_noise(Bl, Bu, K, stream0=9000)
    with T.rng_for_step(nz):
        out = S.train_step_grouped(model, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), O.schedule(10), return_outputs=True)
    torch.cuda.synchronize()
    worst_s = max(abs(float(out[k]) - float(g["s0." + k])) / max(abs(float(g["s0." + k])), 1e-6) for k in T.SCALARS)
    worst_t = max(T.rel_err(out[k].float().cpu().numpy(), g["s0." + k]) for k in T.TENSORS if k in out)
    print("bf16 preactresnet18 step: worst scalar %.3e, worst tensor %.3e" % (worst_s, worst_t))
    assert worst_s <= 5e-3 and worst_t <= 3e-2, (worst_s, worst_t)
    # the bf16 gradient of the whole 11 M-parameter network against the fp32 oracle's: the cosine gate of the bf16 step tests
    # (tests/test_dropout_gpu.py::_gate: > 0.93)
    ref, _, pk = oracle_step(*PREACT_STEP)
    grads = param_grads(model)
    fa = torch.cat([grads[k].double().flatten() for k in pk if not k.endswith("conv0.bias")])
    fb = torch.cat([ref["grads"][k].double().flatten() for k in pk if not k.endswith("conv0.bias")])
    cos = float(fa @ fb / fa.norm() / fb.norm())
    print("bf16 preactresnet18 step: gradient cosine against the fp32 oracle %.5f" % cos)
    assert cos > 0.93, cos


@pytest.mark.parametrize("name", ["preactresnet18", "preactresnet34"])
def test_eval_forward_matches_reference_golden(name):
    g = T.load("ref_eval_" + name.replace("resnet", ""))
    model = make_model(name, "fp32", _state(name)).eval()
    il, ll, iu, lu = C.make_batch(4, 4, 10)
    nz = C.make_noise(4, 4, 10)
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k}
    with torch.no_grad(), T.scripted_rng(randn=[nz["eps3"]], rand=[nz["u3"]]):
        rec, mu, ls, la = model(iu.cuda())
    for k, v in (("rec", rec), ("mu", mu), ("ls", ls), ("la", la)):
        assert T.rel_err(v.float().cpu().numpy(), g[k]) < FP32_TOL, k
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "eval forward must not touch running stats"


def test_preactresnet34_step_matches_oracle():
    name, K, B = "preactresnet34", 10, 8
    out_o, st_o, pk = oracle_step(name, K, B, B)
    model = make_model(name, "fp32", _state(name))
    elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
    il, ll, iu, lu = C.make_batch(B, B, K, stream0=7000)
    nz = C.make_noise(B, B, K, stream0=9000)
    with T.rng_for_step(nz):
        out = S.train_step_grouped(model, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), O.schedule(10), return_outputs=True)
    torch.cuda.synchronize()
    for k in T.SCALARS:
        ref = float(out_o[k])
        assert abs(float(out[k]) - ref) <= FP32_TOL * max(abs(ref), 1e-6), (k, float(out[k]), ref)
    for k in T.TENSORS:
        if k in out:
            assert T.rel_err(out[k].float().cpu().numpy(), out_o[k].numpy()) < FP32_TOL, k
    grads = param_grads(model)
    gn = np.array([float(grads[k].double().norm()) for k in pk])
    gr = out_o["grad_norm"]
    bad = np.abs(gn - gr) > 1e-2 * gr + 1e-4 * gr.max()
    assert not bad.any(), [(pk[i], gn[i], gr[i]) for i in np.nonzero(bad)[0][:5]]


def test_m2_step_matches_oracle():
    name, K, B = "preactresnet18", 10, 8
    il, ll, iu, lu = C.make_batch(B, B, K, stream0=7300)
    nz = C.make_noise(B, B, K, stream0=9300)
    sch = O.schedule(10)
    with P.patched():
        st_o = C.make_state(name, K=K)
        for k in st_o:
            if O.is_param(k):
                st_o[k].requires_grad_(True)
        ref = O.m2_step(st_o, name, il, ll, iu, lu, nz, sch)
    model = make_model(name, "fp32", _state(name))
    elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
    with T.scripted_rng(randn=[nz["eps1"], nz["eps3"]], rand=[nz["u3"]]):
        out = S.m2_train_step(model, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), lu.cuda(), sch, return_outputs=True)
    torch.cuda.synchronize()
    for k in ("recon_l", "klc_l", "kld_l", "recon_u", "klc_u", "kld_u", "disc_post_l", "kl_inference", "loss_sup", "loss_unsup"):
        r = float(ref[k])
        assert abs(float(out[k]) - r) <= FP32_TOL * max(abs(r), 1e-6), (k, float(out[k]), r)
    for k in ("rec1", "mu1", "ls1", "la1", "rec3", "mu3", "ls3", "la3"):
        assert T.rel_err(out[k].float().cpu().numpy(), ref[k].numpy()) < FP32_TOL, k
    grads = param_grads(model)
    pk = [k for k in st_o if O.is_param(k)]
    gn = np.array([float(grads[k].double().norm()) for k in pk])
    gr = np.array([float(st_o[k].grad.double().norm()) for k in pk])
    assert not (np.abs(gn - gr) > 1e-2 * gr + 1e-4 * gr.max()).any()


def test_deterministic_mode_is_bit_identical_and_right():
    name, K, B = PREACT_STEP[0], 10, 8
    g = T.load("ref_step_preact18_br")
    il, ll, iu, lu = C.make_batch(B, B, K, stream0=7000)
    nz = C.make_noise(B, B, K, stream0=9000)
    flats = []
    with L.options(deterministic=1):
        for _ in range(2):
            model = make_model(name, "fp32", _state(name))
            elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
            with T.rng_for_step(nz):
                out = S.train_step_grouped(model, elbo, cls, None, il.cuda(), ll.cuda(), iu.cuda(), O.schedule(10), return_outputs=True)
            torch.cuda.synchronize()
            flats.append(model.flat_parameters()[1].detach().clone())
            for k in T.SCALARS:
                ref = float(g["s0." + k])
                assert abs(float(out[k]) - ref) <= FP32_TOL * max(abs(ref), 1e-6), (k, float(out[k]), ref)
    assert torch.equal(flats[0], flats[1])


def test_dropout_step_matches_masked_oracle(monkeypatch):
    """drop_rate = 0.3 (nn.Dropout between conv1 and norm2, preactresnet.py:33): the sequential step against the oracle whose norm2
    inputs are multiplied by the SAME masks, regenerated from the keys each forward recorded (tests/test_dropout_gpu.py's
    MaskedOracle, comparison and fp32 gates: losses / tensors 1e-3, per-parameter gradients 1.5e-2 against the fp64 run, running
    statistics 1e-3, four BatchNorm updates) -- and the eval-mode forward is the drop_rate = 0 model's, bit for bit."""
    from tests.test_dropout_gpu import MaskedOracle, _compare, _gate, _cast
    name, K, B = "preactresnet18", 10, 8
    il, ll, iu, lu = C.make_batch(B, B, K, stream0=7000)
    nz = C.make_noise(B, B, K, stream0=9000)
    sch = O.schedule(10)
    model = make_model(name, "fp32", _state(name), dp=True, drop_rate=0.3)
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
        mo = MaskedOracle(monkeypatch, model._plan, keys, p=0.3)
        with P.patched():
            st_o = C.make_state(name, K=K)
            for k in st_o:
                if st_o[k].dtype.is_floating_point:
                    st_o[k] = st_o[k].to(dt)
                if O.is_param(k):
                    st_o[k].requires_grad_(True)
            refs[dt] = (st_o, O.train_step(st_o, name, il.to(dt), ll, iu.to(dt), _cast(nz, dt), sch, bce=True))
        assert mo.used_all()
        monkeypatch.undo()
    m = _compare(model, out, refs[torch.float32][1], refs[torch.float32][0], refs[torch.float64][0], T.SCALARS, T.TENSORS)
    print("preactresnet18, dropout 0.3, fp32: cosine %.6f, worst gradient tensor %.3e (%s), worst scalar %.3e, worst tensor %.3e, "
          "running %.3e" % (m["cos"], m["worst"][0], m["worst"][1], max(m["scalar"].values()), max(m["tensor"].values()), m["running"]))
    _gate(m, "fp32", 1e-3, 1e-3, 1.5e-2, 4)
    # eval mode: dropout is the identity
    outs = []
    for p_ in (0.0, 0.3):
        me = make_model(name, "fp32", _state(name), drop_rate=p_).eval()
        with torch.no_grad(), T.scripted_rng(randn=[nz["eps3"]], rand=[nz["u3"]]):
            outs.append([t.clone() for t in me(iu.cuda())])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_graphed_step_equals_eager_step():
    """GraphedTrainStep (the grouped step captured into a hipGraph and replayed) against the eager grouped step with the device
    draws frozen and a fixed summation order, as tests/test_dropout_gpu.py::test_graphed_step_with_dropout_equals_eager_step: after
    two warm-up steps and two replays every parameter and BatchNorm buffer equals the eager run's (2e-6), the counters 4 per step.
    The eager step is held to the reference and the oracle by the tests above."""
    from shot_vae_amd.train import GraphedTrainStep, DeviceRng, train_step_grouped
    name, K, Bl, Bu = "preactresnet18", 10, 8, 8
    state = _state(name)
    il, ll, iu, lu = C.make_batch(Bl, Bu, K)
    il, ll, iu = il.cuda(), ll.cuda(), iu.cuda()
    gen = torch.Generator(device="cuda").manual_seed(7)
    frozen = {}
    real = (torch.randn, torch.rand)

    def fixed(kind, fn):
        def f(*a, **kw):
            key = (kind,) + tuple(x if not isinstance(x, torch.Size) else tuple(x) for x in a)
            if key not in frozen:
                frozen[key] = fn(*a, device="cuda", generator=gen)
            return frozen[key].clone()
        return f

    torch.randn, torch.rand = fixed("n", real[0]), fixed("u", real[1])
    det = L.options(deterministic=1)
    det.__enter__()
    try:
        sch = O.schedule(10)
        elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
        m1, m2 = make_model(name, "fp32", state), make_model(name, "fp32", state)
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
        sa, sb = m1.state_dict(), m2.state_dict()
        moved = T.rel_err(sa["feature_extractor.encoder.block4.preact_block.unit2.f_block.conv2.weight"].cpu().numpy(),
                          state["feature_extractor.encoder.block4.preact_block.unit2.f_block.conv2.weight"].numpy())
        assert moved > 1e-4, moved
        for k in sa:
            if sa[k].dtype.is_floating_point:
                assert T.rel_err(sb[k].cpu().numpy(), sa[k].cpu().numpy()) < 2e-6, k
            else:
                assert int(sa[k]) == int(sb[k]) == 4 * (warm + steps), k
    finally:
        det.__exit__(None, None, None)
        torch.randn, torch.rand = real


@pytest.mark.timeout(900)
def test_two_rank_gloo_step_equals_single_process_over_both_shards(tmp_path):
    """Two ranks on one GPU over gloo (the decoder-first bucket, the flat all-reduce over the four-stage plan, 1 / world in the SGD
    kernel), two steps, against ONE process that runs both shards with their own BatchNorm statistics and steps on the mean: the
    worker of tests/test_dropout_gpu.py with the PreActResNet-18 encoder and drop_rate = 0, its gates (1e-5).  The single-process
    grouped step is held to the reference and the oracle by the tests above."""
    from tests.test_dropout_gpu import DP_EQUIV_WORKER, ROOT, _run_two_ranks
    src = DP_EQUIV_WORKER.replace('"wideresnet-10-1", num_input_channels=3, drop_rate=0.3', '"preactresnet18", num_input_channels=3, drop_rate=0')
    assert '"preactresnet18"' in src and "K, B = 10, 16" in src
    script = tmp_path / "equiv_preact.py"
    script.write_text(src % ROOT)
    res = _run_two_ranks(script, port0=30750, world=2)
    print("two ranks, preactresnet18:", res)
    assert res["moved"] > 1e-4, res
    assert res["rel_param_diff"] < 1e-5, res
    assert res["rel_buf_diff"] < 1e-5, res
