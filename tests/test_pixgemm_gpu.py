"""The per-pixel GEMM kernel (pixgemm.hip) for ConvTranspose2d(4, 2, 1) on maps of up to 4 x 4 pixels and its data gradient, against
torch conv_transpose2d / conv2d in fp64 on the bf16-quantised operands, at the bf16 tolerance of
test_kernels_gpu.py::test_convT_forward_and_dgrad -- on the new kernel (default tile choice and the widest tiles) and with
SV_K_PIXGEMM disabled (the gather-GEMM the layers took before); the label of the launch says which kernel ran."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from shot_vae_amd import _lib as L                                                          # noqa: E402
from shot_vae_amd import geometry as G                                                      # noqa: E402
from tests.test_kernels_gpu import DT, SENTINEL, bq, nchw, nhwc, rel, repack, run_igemm     # noqa: E402

TOL = DT["bf16"][2]
SUM_TOL = max(TOL, 1e-3) * 3
PIXEL = "sv_igemm(pixel)"
SLOPE = 0.01

# Every H with every (Cin, N), the batches and group counts rotating: a ragged image tile (6, 37), a second 128-image tile plus a
# ragged rest (130), a K tail of one 32-channel chunk behind a 64-deep one (96), channel tiles that are not full (32, 192 on 64- and
# 128-wide tiles), one and three BatchNorm groups.
SHAPES = [(64, 32), (96, 128), (128, 192)]
BATCHES = [6, 37, 130]
CASES = [(h, cin, n, BATCHES[(i + j) % 3], 3 if (i + 2 * j) % 3 == 1 else 1)
         for i, h in enumerate((1, 2, 4)) for j, (cin, n) in enumerate(SHAPES)]
# default: the dispatcher's tile choice (64 x 64 for these small products); widest: 128 x 128 / 128 x 64; off: the kernel disabled.
# The LDS-halo kernels, which come first in the dispatcher and take the thin 4x4 -> 8x8 ConvTranspose (N <= 64, Cin <= 128), are
# switched off throughout: the comparison is the per-pixel kernel against the gather-GEMM on every case.
HALO = L.K_HALO | L.K_HALOP
MODES = {"default": dict(disable=HALO), "widest": dict(disable=HALO, wide_min_blocks=1), "off": dict(disable=HALO | L.K_PIXGEMM)}


@functools.lru_cache(maxsize=None)
def reference(h, cin, n, b, groups):
    """operands (bf16 values) and fp64 results of one layer, computed once per case"""
    torch.manual_seed(1000 * h + cin + b)
    gb = groups * b
    x = bq(torch.randn(gb, cin, h, h), "bf16")
    w = bq(torch.randn(cin, n, 4, 4) / (cin * 4) ** 0.5, "bf16")
    y = F.conv_transpose2d(x.double(), w.double(), None, 2, 1)
    dy = bq(torch.randn(gb, n, 2 * h, 2 * h), "bf16")
    da = F.conv2d(dy.double(), w.double(), None, 2, 1)
    # the activation-backward epilogue of the data gradient: the layer's raw input and its BatchNorm's vectors, per group
    xraw = bq(torch.randn(gb, cin, h, h), "bf16")
    vec = dict(scale=torch.rand(groups, cin) + 0.5, shift=torch.randn(groups, cin) * 0.3, mean=torch.randn(groups, cin) * 0.1,
               rstd=torch.rand(groups, cin) + 0.5)
    per = lambda v: v.repeat_interleave(b, 0)[:, :, None, None]
    u = xraw * per(vec["scale"]) + per(vec["shift"])                       # fp32, as the kernel forms it
    gref = da * torch.where(u > 0, 1.0, SLOPE).double()
    xh = (xraw.double() - per(vec["mean"]).double()) * per(vec["rstd"]).double()
    grp = lambda t: t.view(groups, b, *t.shape[1:])
    sums_f = torch.cat([grp(y).sum((1, 3, 4)), (grp(y) ** 2).sum((1, 3, 4))], 1)
    sums_b = torch.cat([grp(gref).sum((1, 3, 4)), grp(gref * xh).sum((1, 3, 4))], 1)
    master = w.permute(1, 2, 3, 0).reshape(n, 16, cin).contiguous()
    return dict(x=x, w=w, y=y, dy=dy, gref=gref, xraw=xraw, vec=vec, sums_f=sums_f, sums_b=sums_b, master=master)


def check_label(mode):
    if mode == "off":
        assert L.last_kernel() != PIXEL
    else:
        assert L.last_kernel() == PIXEL, L.last_kernel()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("h,cin,n,b,groups", CASES)
def test_forward_with_statistics(h, cin, n, b, groups, mode):
    r = reference(h, cin, n, b, groups)
    g = G.convT_like(b, h, h, cin, n, 4, 2, 1)
    with L.options(**MODES[mode]):
        out, sums = run_igemm(g, "bf16", nhwc(r["x"]), repack(r["master"], g, False, "bf16"), stats=True, groups=groups)
        check_label(mode)
    e_out, e_sum = rel(nchw(out), r["y"]), rel(sums.view(groups, 2 * n), r["sums_f"])
    print("forward", (h, cin, n, b, groups), mode, "out %.3g sums %.3g" % (e_out, e_sum))
    assert e_out < TOL
    assert e_sum < SUM_TOL
    for grp in range(groups):                      # each group against its own statistics
        assert rel(sums.view(groups, 2 * n)[grp], r["sums_f"][grp]) < SUM_TOL


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("h,cin,n,b,groups", CASES)
def test_data_gradient_with_activation_backward(h, cin, n, b, groups, mode):
    r = reference(h, cin, n, b, groups)
    gd = G.conv_like(b, 2 * h, 2 * h, n, cin, 4, 2, 1)
    ex = dict(x=nhwc(r["xraw"]), slope=SLOPE, **r["vec"])
    with L.options(**MODES[mode]):
        out, sums = run_igemm(gd, "bf16", nhwc(r["dy"]), repack(r["master"], gd, True, "bf16"), ex=ex, groups=groups)
        check_label(mode)
    e_out, e_sum = rel(nchw(out), r["gref"]), rel(sums.view(groups, 2 * cin), r["sums_b"])
    print("dgrad", (h, cin, n, b, groups), mode, "out %.3g bsums %.3g" % (e_out, e_sum))
    assert e_out < TOL
    for grp in range(groups):
        assert rel(sums.view(groups, 2 * cin)[grp, :cin], r["sums_b"][grp, :cin]) < SUM_TOL
        assert rel(sums.view(groups, 2 * cin)[grp, cin:], r["sums_b"][grp, cin:]) < SUM_TOL


@pytest.mark.parametrize("mode", ["default", "off"])
def test_plain_data_gradient_and_padded_leading_dimensions(mode):
    """ldx / ldo wider than the channel counts: NaN columns in the input are not read, the caller's output columns are not written"""
    h, cin, n, b = 2, 96, 128, 37
    r = reference(h, cin, n, b, 1)
    g = G.convT_like(b, h, h, cin, n, 4, 2, 1, ldx=cin + 8, ldo=n + 12)
    gd = G.conv_like(b, 2 * h, 2 * h, n, cin, 4, 2, 1, ldx=n + 16, ldo=cin + 4)
    with L.options(**MODES[mode]):
        info = {}
        out, sums = run_igemm(g, "bf16", nhwc(r["x"]), repack(r["master"], g, False, "bf16"), stats=True, info=info)
        check_label(mode)
        assert rel(nchw(out[..., :n]), r["y"]) < TOL and rel(sums, r["sums_f"][0]) < SUM_TOL
        assert (out[..., n:] == SENTINEL).all() and (info["lo"] == SENTINEL).all() and (info["hi"] == SENTINEL).all()
        info = {}
        out, _ = run_igemm(gd, "bf16", nhwc(r["dy"]), repack(r["master"], gd, True, "bf16"), info=info)
        check_label(mode)
        da = F.conv2d(r["dy"].double(), r["w"].double(), None, 2, 1)
        assert rel(nchw(out[..., :cin]), da) < TOL
        assert (out[..., cin:] == SENTINEL).all() and (info["lo"] == SENTINEL).all() and (info["hi"] == SENTINEL).all()


@pytest.mark.parametrize("what", ["f32", "prologue", "bias", "H16"])
def test_declined_launches_still_match(what):
    """fp32, a load prologue, a bias and a 16 x 16 map are not the kernel's: the try declines and the launch runs as before"""
    h, cin, n, b = (16 if what == "H16" else 2), 64, 32, 6
    dt = "f32" if what == "f32" else "bf16"
    torch.manual_seed(7)
    x = bq(torch.randn(b, cin, h, h), dt)
    w = bq(torch.randn(cin, n, 4, 4) / (cin * 4) ** 0.5, dt)
    scale, shift, bias = torch.rand(cin) + 0.5, torch.randn(cin) * 0.3, torch.randn(n)
    a = bq(F.relu(x * scale[None, :, None, None] + shift[None, :, None, None]), dt) if what == "prologue" else x
    y = F.conv_transpose2d(a.double(), w.double(), bias.double() if what == "bias" else None, 2, 1)
    g = G.convT_like(b, h, h, cin, n, 4, 2, 1)
    master = w.permute(1, 2, 3, 0).reshape(n, 16, cin).contiguous()
    out, sums = run_igemm(g, dt, nhwc(x), repack(master, g, False, dt), pro=(scale, shift, 0.0) if what == "prologue" else None,
                          bias=bias if what == "bias" else None, stats=True)
    assert L.last_kernel() != PIXEL and L.last_kernel() != ""
    assert rel(nchw(out), y) < DT[dt][2]
    assert rel(sums[:n], y.sum((0, 2, 3))) < max(DT[dt][2], 1e-3) * 3
    gd = G.conv_like(b, 2 * h, 2 * h, n, cin, 4, 2, 1)
    if what in ("f32", "H16"):
        dy = bq(torch.randn(b, n, 2 * h, 2 * h), dt)
        out, _ = run_igemm(gd, dt, nhwc(dy), repack(master, gd, True, dt))
        assert L.last_kernel() != PIXEL
        assert rel(nchw(out), F.conv2d(dy.double(), w.double(), None, 2, 1)) < DT[dt][2]


def test_grid_is_the_table_s_pixels_times_the_tiles():
    """sv_debug_pixgemm_table and the launch agree: one block per (output pixel of the table, image tile, channel tile), and
    sv_debug_last_kernel names the kernel that a real launch -- not the grid query in front of it -- took"""
    import ctypes as C
    h, cin, n, b = 4, 96, 128, 6
    r = reference(h, cin, n, b, 3)
    g = G.convT_like(b, h, h, cin, n, 4, 2, 1)
    npix, pixels, taps = C.c_int(0), (C.c_int * (64 * 4))(), (C.c_int * (64 * 16 * 4))()
    L.call("sv_debug_pixgemm_table", C.byref(g), C.byref(npix), pixels, taps)
    assert npix.value == 4 * h * h
    with L.options(**MODES["off"]):
        run_igemm(g, "bf16", nhwc(r["x"]), repack(r["master"], g, False, "bf16"), groups=3)
    buf = C.create_string_buffer(64)
    L.call("sv_debug_last_kernel", buf, 64)
    assert buf.value.decode() == L.last_kernel() != PIXEL
    with L.options(**MODES["widest"]):          # 128 x 128 tiles: one image tile, one channel tile
        info = {}
        run_igemm(g, "bf16", nhwc(r["x"]), repack(r["master"], g, False, "bf16"), groups=3, info=info)
    L.call("sv_debug_last_kernel", buf, 64)
    assert buf.value.decode() == PIXEL and info["blocks"] == npix.value


@pytest.mark.parametrize("h,cin,n,b,groups", [CASES[1], CASES[8]])
def test_outputs_equal_the_gather_gemm_bit_for_bit(h, cin, n, b, groups):
    """Same products in the same order per output element -- the phase's taps in pack order, 32 channels per MFMA, channels
    ascending; the padding taps the gather-GEMM also multiplies add exact zeros -- so the two kernels' outputs are EQUAL; only
    the grouping of the fp32 partial sums behind the statistics differs."""
    r = reference(h, cin, n, b, groups)
    g = G.convT_like(b, h, h, cin, n, 4, 2, 1)
    gd = G.conv_like(b, 2 * h, 2 * h, n, cin, 4, 2, 1)
    ex = dict(x=nhwc(r["xraw"]), slope=SLOPE, **r["vec"])
    res = {}
    for mode in ("default", "widest", "off"):
        with L.options(**MODES[mode]):
            f, _ = run_igemm(g, "bf16", nhwc(r["x"]), repack(r["master"], g, False, "bf16"), stats=True, groups=groups)
            d, _ = run_igemm(gd, "bf16", nhwc(r["dy"]), repack(r["master"], gd, True, "bf16"), ex=ex, groups=groups)
            check_label(mode)
        res[mode] = (f, d)
    for mode in ("default", "widest"):
        assert torch.equal(res[mode][0], res["off"][0]) and torch.equal(res[mode][1], res["off"][1]), mode
