"""Exact integer parity of the convolution family on a real MI355X: sv_igemm (every kernel label sv_igemm_launch can record),
sv_wgrad_ex (the generic kernel and each specialised one, switched on and off) and sv_bwd3x3 (one-, two- and three-tensor form)
on the small-integer operands of tests/_exact.py, compared with `==` against torch's float64 conv2d / conv_transpose2d /
conv2d_weight.  There is no tolerance in this file: the operands are built so that every product and every partial sum is exact in
fp32 in any order and every stored output is its own bf16 rounding (tests/_exact.py `preconditions`, proven for every case of the
tables by tests/test_conv_exact_cpu.py), so a correct kernel owes equality, and a mismatch names an (image, row, column, channel).

sv_igemm: `L.last_kernel()` must equal the label the table expects -- a case the dispatcher reroutes fails instead of silently
testing another kernel.  Per launch: `out` whole, `stats` / `bsums` with the replicas summed, the guard bands around the output.
sv_wgrad_ex: the launches have no label; shapes and switches are taken verbatim from the existing test of each kernel (the `source`
column of tests/_exact.py WGRAD: test_conv_wgrad, test_thin_layers_wgrad, test_thin_4x4_stride2_wgrad, test_banded_stride2_wgrad,
test_tap_fused_wgrad_conv / _convT, test_wide_cooperative_wgrad of tests/test_kernels_gpu.py and test_map4_wgrad of
tests/test_preact_gpu.py), with the kernel dispatched and switched off; dw starts from 3, accumulates one call without and one
with the (NaN-filled) slab workspace and must equal 3 + 2 * reference.
sv_bwd3x3: out, bsums, dw and dy_out.  The fold_* form divides and takes a reciprocal square root: not exact, it stays with
tests/test_fused_bwd_gpu.py::test_fold_derives_the_coefficients_of_sv_bn_bwd_affine."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from shot_vae_amd import _lib as L          # noqa: E402
from shot_vae_amd import geometry as G      # noqa: E402
from tests import _exact as E               # noqa: E402
from tests.test_kernels_gpu import ACC, DT, SENTINEL, dev, nhwc, repack, run_igemm, st   # noqa: E402


def geometry(c):
    """-> the launch's sv_geom, whether the pack is the transposed (data-gradient) one"""
    if c.kind == "conv":
        return G.conv_like(c.B, c.H, c.H, c.Cin, c.N, c.k, c.stride, c.pad), False
    if c.kind == "convT":
        return G.convT_like(c.B, c.H, c.H, c.Cin, c.N, 4, 2, 1), False
    if c.kind == "conv_dgrad":
        return G.convT_like(c.B, c.Ho, c.Ho, c.N, c.Cin, c.k, c.stride, c.pad), True
    assert c.kind == "convT_dgrad"
    return G.conv_like(c.B, c.Ho, c.Ho, c.N, c.Cin, 4, 2, 1), True


@pytest.mark.parametrize("name,label,dt,case,opts", E.IGEMM, ids=[r[0] for r in E.IGEMM])
def test_igemm_equals_float64(name, label, dt, case, opts):
    b = E.build(case)
    g, transpose = geometry(case)
    wp = repack(b.master.float(), g, transpose, dt)
    info = {}
    with L.options(**opts):
        if case.kind in ("conv", "convT"):
            out, sums = run_igemm(g, dt, nhwc(b.x), wp, pro=b.pro, bias=b.bias, residual=None if b.res is None else nhwc(b.res),
                                  stats=case.stats, groups=case.groups, info=info)
        else:
            ex = None if b.exd is None else dict(b.exd, x=nhwc(b.exd["x"]))
            out, sums = run_igemm(g, dt, nhwc(b.dy), wp, ex=ex, groups=case.groups, info=info)
        ran = L.last_kernel()
    assert ran == label, (name, "the dispatcher took %r, the table expects %r" % (ran, label))
    E.assert_equal(out, nhwc(b.y), name + " out")
    if sums is not None:
        E.assert_equal(sums.view(case.groups, -1), b.sums, name + (" stats" if case.kind in ("conv", "convT") else " bsums"))
    assert bool((info["lo"] == SENTINEL).all()) and bool((info["hi"] == SENTINEL).all()), (name, "store outside the output tensor")


_WS = {}


def workspace():
    """16 Mi floats of NaN: a slab workspace's contents are irrelevant on entry"""
    if "ws" not in _WS:
        _WS["ws"] = torch.empty(16 * 1024 * 1024, device=dev())
    _WS["ws"].fill_(float("nan"))
    return _WS["ws"]


def run_wgrad(c, b, dt, use_tr, opts, budget):
    """dw = DW0, then two accumulating sv_wgrad_ex calls: without and with the slab workspace"""
    code, tdt, _ = DT[dt]
    d = dev()
    T = c.k * c.k
    g = G.convT_like(c.B, c.H, c.H, c.Cin, c.N, 4, 2, 1) if c.kind == "wgradT" else G.conv_like(c.B, c.H, c.H, c.Cin, c.N, c.k, c.stride, c.pad)
    xd, dyd = nhwc(b.x).to(d, tdt).contiguous(), nhwc(b.dy).to(d, tdt).contiguous()
    dw = torch.full((c.N, T, c.Cin), E.DW0, device=d)
    ws = workspace()
    if b.pro is not None:
        sc, sh = b.pro[0].to(d).float().contiguous(), b.pro[1].to(d).float().contiguous()
    with L.options(**opts):
        for with_ws in (False, True):
            a = L.SvWgradArgs()
            a.x, a.dy, a.dw = xd.data_ptr(), dyd.data_ptr(), dw.data_ptr()
            if b.pro is not None:
                a.pro_scale, a.pro_shift, a.pro_slope = sc.data_ptr(), sh.data_ptr(), b.pro[2]
            a.splits, a.use_tr, a.groups, a.block_budget = 0, use_tr, c.groups, budget
            if with_ws:
                a.ws, a.ws_elems = ws.data_ptr(), ws.numel()
            L.call("sv_wgrad_ex", C.byref(g), code, C.byref(a), st())
        torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize("name,dt,use_tr,case,on,off,budget,source", E.WGRAD, ids=[r[0] for r in E.WGRAD])
def test_wgrad_equals_float64(name, dt, use_tr, case, on, off, budget, source):
    b = E.build(case)
    want = E.DW0 + 2 * b.dw
    E.assert_equal(run_wgrad(case, b, dt, use_tr, on, budget), want, name + " dw")
    if off is not None:
        E.assert_equal(run_wgrad(case, b, dt, use_tr, off, budget), want, name + " dw (kernel switched off)")


@pytest.mark.parametrize("name,case,budget", E.BWD, ids=[r[0] for r in E.BWD])
def test_bwd3x3_equals_float64(name, case, budget):
    c, b = case, E.build(case)
    d, bf = dev(), torch.bfloat16
    Cc, Gn, R = c.Cin, c.groups, 4
    gd = G.convT_like(c.B, c.H, c.H, Cc, Cc, 3, 1, 1)
    wd = repack(b.master.float(), gd, True, "bf16")

    def to_dev(t):
        return nhwc(t).to(d, bf).contiguous()

    def vec(t):
        return t.to(d).float().contiguous()

    dy, x = to_dev(b.dy), to_dev(b.exd["x"])
    out = torch.full_like(x, SENTINEL)
    bs = torch.zeros(Gn, R, 2 * Cc, device=d, dtype=ACC)
    dw = torch.full((Cc, 9, Cc), E.DW0, device=d)
    ws = workspace()
    keep = [vec(b.exd[k]) for k in ("scale", "shift", "mean", "rstd")]
    a = L.SvBwd3x3Args()
    a.dy, a.x, a.w, a.out = dy.data_ptr(), x.data_ptr(), wd.data_ptr(), out.data_ptr()
    a.x_scale, a.x_shift, a.x_mean, a.x_rstd = (t.data_ptr() for t in keep)
    a.x_slope = E.SLOPE
    if c.form >= 1:
        dy2 = to_dev(b.dy2)
        coef = [vec(t) for t in b.coef]
        a.dy2, a.dy_scale, a.dy_scale2, a.dy_shift = dy2.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(), coef[2].data_ptr()
    if c.form == 2:
        dy3 = to_dev(b.dy3)
        dy_out = torch.full_like(dy, 5.0)
        a.dy3, a.dy_out = dy3.data_ptr(), dy_out.data_ptr()
    a.bsums, a.replicas, a.groups, a.dw, a.ws, a.ws_elems, a.block_budget = bs.data_ptr(), R, Gn, dw.data_ptr(), ws.data_ptr(), ws.numel(), budget
    L.call("sv_bwd3x3", C.byref(gd), L.SV_BF16, C.byref(a), st())
    torch.cuda.synchronize()
    E.assert_equal(out.float().cpu(), nhwc(b.y), name + " out")
    E.assert_equal(bs.sum(1).cpu(), b.sums, name + " bsums")
    E.assert_equal(dw.cpu(), E.DW0 + b.dw, name + " dw")
    if c.form == 2:
        E.assert_equal(dy_out.float().cpu(), nhwc(b.eff), name + " dy_out")
