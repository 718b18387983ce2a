"""The conv entry points off the model's geometry: sv_igemm with padded leading dimensions (ldo > N, ldx > Cin) through every
specialised kernel and the generic gather-GEMM, and sv_igemm / sv_wgrad_ex on rectangular and odd-sized maps -- against torch's
float64 conv2d / conv_transpose2d / conv2d_weight on the CPU, fed the operands rounded to the storage type (and the activated
prologue output rounded too).  Tolerances: DT of tests/test_kernels_gpu.py (2e-4 of the tensor scale in fp32, 2.5e-2 in bf16,
max(tol, 1e-3) * 3 for the channel sums) -- the same kernels and operand scales as the parity tests there.

The leading-dimension contract (include/shotvae_hip.h, sv_geom), per padded launch:
  (a) out[..., :N] matches the reference;
  (b) columns [N, ldo) of every pixel row and a band of sentinel elements in front of and behind the output keep their bits;
  (c) the `stats` sums (forward) / the `bsums` of the `ex` epilogue (data gradient) match, residual and raw tensor padded too;
  (d) out[..., :N] has the bits of the same launch with ldo == N (the tile decomposition does not depend on ld).
Every family runs with its kernel on and off (the K_* bit the dispatcher tests), both against the reference; `took` records whether
the bit made a difference -- another grid (sv_igemm_query_blocks) or other bits -- and every test asserts that one of its padded
launches did (`demonstrated`), so a case cannot silently run the generic kernel twice.  Where neither can differ (same block count,
same accumulation order on both sides of the switch) the guard line that takes the case is cited in CITED.  Guards read for the
case tables (what they require of ld):
  conv3x3.hip  conv3x3_covers      ldx == Cin; ldo unchecked (sv_igemm: ldo % 4)        -> pad 4 / 8 / 24
  conv3x3w.hip sv_conv3x3w_try     ldo % 8 (`g->ldo % 8 != 0` declines)                 -> pad 8 / 24
  conv3x3x.hip sv_conv3x3x_try     behind sv_conv3x3w_try                               -> pad 8 / 24
  sconv.hip    sv_sconv_try        ldx == Cin, ldo % 4                                  -> pad 4 / 8 / 24
  thconv.hip   sv_thconv_try       ldx == Cin, ldo % 8                                  -> pad 8 / 24
  pconv.hip    sv_pconv_try        ldx == Cin, ldo % 8                                  -> pad 8 / 24
  dconv.hip    sv_dconv_try        ldx == 16, ldo % 4                                   -> pad 4 / 8 / 24
  tconv.hip    sv_tconvr_try       ldx == Cin; ldo % 4 (128 -> 64, 64 -> 32 ex), ldo % 8 (64 -> 16 forward)
  halo.hip     sv_halo_try         ldx == Cin; ldo unchecked                            -> pad 4 / 8 / 24
No (d) waiver: every guard above admits the padded geometry of its cases.

Measured on MI355X (maxima over all families, relative to the tensor scale; per family in DESIGN.md, "Off-model geometry"):
fp32 out 1.4e-6, sums 1.0e-6, dw 3.0e-7; bf16 out 3.6e-3, sums 3.7e-7, dw 1.7e-5.  No kernel or guard had to change."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from shot_vae_amd import _lib as L          # noqa: E402
from shot_vae_amd import geometry as G      # noqa: E402
from tests.test_kernels_gpu import ACC, DT, SENTINEL, bq, dev, nhwc, rel, repack, run_igemm, st   # noqa: E402

F64 = torch.float64
SLOPE = 0.01


def sums_tol(dt):
    return max(DT[dt][2], 1e-3) * 3


def report(family, dt, what, value):
    """every measured figure goes to stdout before it is asserted on (pytest -s / the captured output of a failure)"""
    print("GEOM %-14s %-4s %-5s %.3e" % (family, dt, what, value))


class Problem:
    """One conv-like layer with random operands (rounded to the storage type) and its float64 reference, built once and shared
    by every launch variant of a case.  kind: "conv" (Conv2d forward), "convT" (ConvTranspose2d(4, 2, 1) forward), "conv_dgrad" /
    "convT_dgrad" (their data gradients, with the activation-backward epilogue when fused).  Cin -> N are the LAYER's channels;
    gin / gout the launch's."""

    def __init__(self, kind, dt, B, Cin, N, H, W, k, stride, pad, groups=1, pro=True, bias=True, res=True, seed=1):
        torch.manual_seed(seed)
        self.kind, self.dt, self.groups, self.B = kind, dt, groups, B
        GB = groups * B
        conv = kind.startswith("conv") and not kind.startswith("convT")
        if conv:
            Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
            w = bq(torch.randn(N, Cin, k, k) / (Cin * k * k) ** 0.5, dt)
            self.master = w.permute(0, 2, 3, 1).reshape(N, k * k, Cin).contiguous()
        else:
            Ho, Wo = 2 * H, 2 * W
            w = bq(torch.randn(Cin, N, 4, 4) / (Cin * 4) ** 0.5, dt)
            self.master = w.permute(1, 2, 3, 0).reshape(N, 16, Cin).contiguous()
        wd = w.to(F64)
        gi = torch.arange(GB) // B

        def per(v):      # [groups][C] coefficients -> [GB, C, 1, 1]
            return v[gi][:, :, None, None]

        if kind in ("conv", "convT"):
            self.gin, self.gout = Cin, N
            x = bq(torch.randn(GB, Cin, H, W), dt)
            self.x = nhwc(x)
            a = x
            self.pro = None
            if pro:
                scale, shift = torch.rand(groups, Cin) + 0.5, torch.randn(groups, Cin) * 0.3
                self.pro = (scale, shift, SLOPE)
                a = bq(F.leaky_relu(x * per(scale) + per(shift), SLOPE), dt)
            self.bias = torch.randn(N) * 0.2 if bias else None
            b64 = None if self.bias is None else self.bias.to(F64)
            y = F.conv2d(a.to(F64), wd, b64, stride, pad) if conv else F.conv_transpose2d(a.to(F64), wd, b64, 2, 1)
            self.res = None
            if res:
                r = bq(torch.randn(GB, N, Ho, Wo), dt)
                self.res = nhwc(r)
                y = y + r.to(F64)
            self.ex = None
            self.geom = (lambda ldx=None, ldo=None: G.conv_like(B, H, W, Cin, N, k, stride, pad, ldx, ldo)) if conv else \
                        (lambda ldx=None, ldo=None: G.convT_like(B, H, W, Cin, N, 4, 2, 1, ldx, ldo))
            self.transpose = False
            ys = y.view(groups, B, N, Ho, Wo)
            self.sums = torch.cat([ys.sum((1, 3, 4)), (ys * ys).sum((1, 3, 4))], 1)
        else:
            # the data gradient maps the layer's output channels (N) back to its input channels (Cin)
            self.gin, self.gout = N, Cin
            dy = bq(torch.randn(GB, N, Ho, Wo), dt)
            self.x = nhwc(dy)
            self.pro = self.bias = self.res = None
            if conv:
                assert H % stride == 0 and W % stride == 0 and Ho == H // stride and Wo == W // stride
                da = F.conv_transpose2d(dy.to(F64), wd, None, stride, pad, output_padding=(H - ((Ho - 1) * stride - 2 * pad + k),
                                                                                             W - ((Wo - 1) * stride - 2 * pad + k)))
                self.geom = lambda ldx=None, ldo=None: G.convT_like(B, Ho, Wo, N, Cin, k, stride, pad, ldx, ldo)
            else:
                da = F.conv2d(dy.to(F64), wd, None, 2, 1)
                self.geom = lambda ldx=None, ldo=None: G.conv_like(B, Ho, Wo, N, Cin, 4, 2, 1, ldx, ldo)
            self.transpose = True
            xraw = bq(torch.randn(GB, Cin, H, W), dt)
            scale, shift = torch.rand(groups, Cin) + 0.5, torch.randn(groups, Cin) * 0.3
            mean, rstd = torch.randn(groups, Cin) * 0.1, torch.rand(groups, Cin) + 0.5
            self.ex = dict(x=nhwc(xraw), scale=scale, shift=shift, mean=mean, rstd=rstd, slope=SLOPE)
            u = xraw * per(scale) + per(shift)                           # (fp32, as the kernels form it)
            y = da * torch.where(u > 0, torch.ones_like(u), torch.full_like(u, SLOPE)).to(F64)
            xh = ((xraw - per(mean)) * per(rstd)).to(F64)
            ys, xs = y.view(groups, B, Cin, H, W), xh.view(groups, B, Cin, H, W)
            self.sums = torch.cat([ys.sum((1, 3, 4)), (ys * xs).sum((1, 3, 4))], 1)
        self.y = nhwc(y)
        self._packs = {}

    def pack(self, g):
        key = tuple((g.phase[i].ntap, g.phase[i].w_off) for i in range(g.nphase))
        if key not in self._packs:
            self._packs[key] = repack(self.master, g, self.transpose, self.dt)
        return self._packs[key]

    def launch(self, ldx_pad=0, ldo_pad=0, stats=True, opts=None, sparse_out=0):
        """-> out [GB, Hout, Wout, ldo], sums [groups][2 gout] or None, info (guard bands, grid)"""
        g = self.geom(self.gin + ldx_pad, self.gout + ldo_pad)
        info = {}
        with L.options(**(opts or {})):
            out, sums = run_igemm(g, self.dt, self.x, self.pack(g), pro=self.pro, bias=self.bias, residual=self.res,
                                  stats=stats and self.ex is None, ex=self.ex, groups=self.groups, sparse_out=sparse_out, info=info)
        if sums is not None:
            sums = sums.view(self.groups, -1)
        return out, sums, info


def check(family, pb, out, sums, info, want_sums=True):
    """(a), (b), (c) of the contract for one launch"""
    n, tol = pb.gout, DT[pb.dt][2]
    assert bool(torch.isfinite(out[..., :n]).all()), (family, "non-finite output")
    for gi in range(pb.groups):
        sl = slice(gi * pb.B, (gi + 1) * pb.B)
        e = rel(out[sl][..., :n], pb.y[sl])
        report(family, pb.dt, "out", e)
        assert e < tol, (family, "out", gi, e)
    assert bool((out[..., n:] == SENTINEL).all()), (family, "columns [N, ldo) were written")
    assert bool((info["lo"] == SENTINEL).all()) and bool((info["hi"] == SENTINEL).all()), (family, "store outside the output tensor")
    if want_sums:
        assert sums is not None
        for gi in range(pb.groups):
            for half in (slice(0, n), slice(n, 2 * n)):
                e = rel(sums[gi, half], pb.sums[gi, half])
                report(family, pb.dt, "sums", e)
                assert e < sums_tol(pb.dt), (family, "sums", gi, e)


def took(family, a, b, what):
    """the two launches (kernel on / off) did not run the same kernel: another grid, or other bits"""
    (out_a, _, info_a), (out_b, _, info_b) = a, b
    hit = info_a["blocks"] != info_b["blocks"] or not torch.equal(out_a, out_b)
    print("GEOM-TOOK %-16s %-34s grid %d / %d, bits %s" % (family, what, info_a["blocks"], info_b["blocks"],
                                                          "equal" if torch.equal(out_a, out_b) else "differ"))
    return hit


def contract(family, pb, pads, on, off, stats=True, identity=True):
    """Padded ldo through the kernel (options `on`) and without it (`off`), each against the reference; the padded result against the
    dense one, bit for bit, under `on`.  -> the number of padded launches whose switch made a difference (took)"""
    n = pb.gout
    what = "%s %s" % (pb.kind, pb.dt)
    dense = pb.launch(0, 0, stats, on)
    check(family, pb, *dense, want_sums=stats)
    hits = 0
    for pad in pads:
        r_on, r_off = pb.launch(0, pad, stats, on), pb.launch(0, pad, stats, off)
        check(family, pb, *r_on, want_sums=stats)
        check(family, pb, *r_off, want_sums=stats)
        hits += took(family, r_on, r_off, "%s ldo = N + %d" % (what, pad))
        if identity:
            assert torch.equal(r_on[0][..., :n], dense[0]), (family, "padded ldo changed the bits of out[..., :N]", pad)
            assert r_on[2]["blocks"] == dense[2]["blocks"], (family, "padded ldo changed the grid", pad)
    return hits


# Cases whose switch changes NEITHER the grid nor a bit: the kernels on both sides of the switch cut the problem into the same number
# of blocks and accumulate in the same order (specialised kernels are bit-equal to the kernels they replace where the
# arithmetic order is the same).  For these the guard line that takes the padded geometry is cited instead.
CITED = {
    ("conv3x3p", (4, 32, 32, 32, 3, 1, 1)):
        "conv3x3.hip sv_conv3x3_try: `!no_persist && dtype == SV_BF16 && (g->Cin == 32 || g->Cin == 64)` (bf16) / `dtype == SV_F32 && "
        "g->Cin == 32` (fp32) -> launch_pw, behind conv3x3_covers (no ldo condition); 32 tiles = 32 blocks in conv3x3_kernel too",
    ("conv3x3w", (8, 128, 128, 8, 3, 1, 1)):
        "conv3x3w.hip sv_conv3x3w_try: `g->ldo % 8 != 0` declines, N % 128 == 0 with two 256-pixel tiles -> bn = 128, launch_w2<4>; "
        "conv3x3_kernel has 4 tiles x 2 channel tiles = the same 8 blocks",
    ("conv3x3x", (4, 160, 160, 8, 3, 1, 1)):
        "conv3x3x.hip sv_conv3x3x_try: `g->N % 160 != 0 || g->Cin % 32 != 0 || g->Cin < 96` declines, else launch_x2 (called from "
        "sv_conv3x3w_try with bn == 160, whose `g->ldo % 8` admits the pad); bit-equal to conv3x3w by construction",
    ("conv3x3x", (3, 160, 320, 32, 3, 1, 1)): "as above",
    ("pconv", (3, 16, 32, 32, 1, 1, 0)):
        "pconv.hip sv_pconv_try: `g->ldx != g->Cin || g->ldo % 8 != 0 || ...` declines, `g->Cin == 16 && g->N == 32` -> "
        "launch_pconv<16, 32>; 96 tiles of 32 positions on 24 blocks, the gather-GEMM has 24 tiles of 128 rows",
}


def demonstrated(family, case, hits):
    """at least one padded-ldo launch of the invocation demonstrably ran the family's kernel -- or its guard line is cited"""
    assert hits > 0 or (family, tuple(case)) in CITED, (family, case, "no padded launch shows that the kernel ran, and no guard is cited")


def poison_ldx(family, pb, opts=None, ldo_pad=0):
    """Columns [Cin, ldx) hold NaN: the result is finite and right, whichever kernel answers (every specialised guard requires
    ldx == Cin, so it is the generic gather-GEMM)."""
    for pad in (8, 24):
        r = pb.launch(pad, ldo_pad, True, opts)
        check(family + "/ldx", pb, *r)


# ------------------------------------------------------------------------------------ 1. padded leading dimensions
@pytest.mark.parametrize("dt,case", [("bf16", (4, 32, 32, 32, 3, 1, 1)), ("bf16", (4, 64, 64, 16, 3, 1, 1)), ("f32", (4, 32, 32, 32, 3, 1, 1))])
def test_ld_conv3x3_persistent(dt, case):
    """conv3x3p (whole weight slab in LDS): the run-time-flag binary (bias), the compile-time forward binary of the step
    (prologue + residual + statistics, no bias) and the data gradient with the `ex` epilogue."""
    B, Cin, N, H, k, s, pd = case
    on, off = {}, dict(disable=L.K_CONV3X3P)
    hits = contract("conv3x3p", Problem("conv", dt, B, Cin, N, H, H, k, s, pd), (4, 8, 24), on, off)
    hits += contract("conv3x3p", Problem("conv", dt, B, Cin, N, H, H, k, s, pd, bias=False, seed=2), (8,), on, off)
    hits += contract("conv3x3p", Problem("conv_dgrad", dt, B, Cin, N, H, H, k, s, pd, seed=3), (4, 8, 24), on, off)
    demonstrated("conv3x3p", case, hits)
    poison_ldx("conv3x3p", Problem("conv", dt, B, Cin, N, H, H, k, s, pd, seed=4))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 32, 96, 16, 3, 1, 1), (2, 160, 160, 8, 3, 1, 1)])
def test_ld_conv3x3_tiled(dt, case):
    """conv3x3_kernel (one 128-pixel tile per block; the persistent kernel switched off) against the gather-GEMM."""
    B, Cin, N, H, k, s, pd = case
    on, off = dict(disable=L.K_CONV3X3P), dict(disable=L.K_CONV3X3)
    hits = contract("conv3x3", Problem("conv", dt, B, Cin, N, H, H, k, s, pd), (4, 8, 24), on, off)
    hits += contract("conv3x3", Problem("conv_dgrad", dt, B, Cin, N, H, H, k, s, pd, seed=3), (4, 8, 24), on, off)
    demonstrated("conv3x3", case, hits)
    poison_ldx("conv3x3", Problem("conv", dt, B, Cin, N, H, H, k, s, pd, seed=4), on)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_ld_conv3x3_map4(dt):
    """the 4 x 4-map instantiation (eight images per tile), off by default: SV_K_MAP4_CONV in the enable mask."""
    case = B, Cin, N, H, k, s, pd = (8, 64, 64, 4, 3, 1, 1)
    on, off = dict(enable=L.K_MAP4_CONV), dict(enable=0)
    hits = contract("conv3x3/4x4", Problem("conv", dt, B, Cin, N, H, H, k, s, pd), (4, 8, 24), on, off)
    hits += contract("conv3x3/4x4", Problem("conv_dgrad", dt, B, Cin, N, H, H, k, s, pd, seed=3), (4, 8, 24), on, off)
    demonstrated("conv3x3/4x4", case, hits)
    poison_ldx("conv3x3/4x4", Problem("conv", dt, B, Cin, N, H, H, k, s, pd, seed=4), on)


@pytest.mark.parametrize("case", [(4, 160, 160, 8, 3, 1, 1), (8, 128, 128, 8, 3, 1, 1)])
def test_ld_conv3x3w(case):
    """the 256-pixel LDS-DMA kernel (160- and 64/128-channel tiles)."""
    B, Cin, N, H, k, s, pd = case
    on, off = dict(wide_min_blocks=1, disable=L.K_CONV3X3X), dict(wide_min_blocks=1, disable=L.K_CONV3X3X | L.K_CONV3X3W)
    hits = contract("conv3x3w", Problem("conv", "bf16", B, Cin, N, H, H, k, s, pd), (8, 24), on, off)
    hits += contract("conv3x3w", Problem("conv_dgrad", "bf16", B, Cin, N, H, H, k, s, pd, seed=3), (8, 24), on, off)
    demonstrated("conv3x3w", case, hits)
    poison_ldx("conv3x3w", Problem("conv", "bf16", B, Cin, N, H, H, k, s, pd, seed=4), on)


@pytest.mark.parametrize("case", [(4, 160, 160, 8, 3, 1, 1), (3, 160, 320, 32, 3, 1, 1)])
def test_ld_conv3x3x(case):
    """the persistent one-wave-per-SIMD variant: the forward binaries (run-time flags with a bias, statistics + residual without)
    and the data gradient (halo by LDS-DMA)."""
    B, Cin, N, H, k, s, pd = case
    on, off = dict(wide_min_blocks=1), dict(wide_min_blocks=1, disable=L.K_CONV3X3X)
    hits = contract("conv3x3x", Problem("conv", "bf16", B, Cin, N, H, H, k, s, pd), (8, 24), on, off)
    hits += contract("conv3x3x", Problem("conv", "bf16", B, Cin, N, H, H, k, s, pd, bias=False, seed=2), (8,), on, off)
    hits += contract("conv3x3x", Problem("conv_dgrad", "bf16", B, Cin, N, H, H, k, s, pd, seed=3), (8, 24), on, off)
    demonstrated("conv3x3x", case, hits)
    poison_ldx("conv3x3x", Problem("conv", "bf16", B, Cin, N, H, H, k, s, pd, seed=4), on)


@pytest.mark.parametrize("case,pro,groups", [((3, 64, 128, 16, 3, 2, 1), True, 1), ((3, 64, 128, 16, 3, 2, 1), False, 1),
                                             ((3, 32, 64, 32, 3, 2, 1), True, 1), ((3, 32, 64, 32, 3, 2, 1), False, 2)])
def test_ld_sconv(case, pro, groups):
    """the register-resident stride-2 3x3 forward (no bias / residual: the guard declines them)."""
    B, Cin, N, H, k, s, pd = case
    pb = Problem("conv", "bf16", B, Cin, N, H, H, k, s, pd, groups=groups, pro=pro, bias=False, res=False)
    demonstrated("sconv", case, contract("sconv", pb, (4, 8, 24), {}, dict(disable=L.K_SCONV)))
    poison_ldx("sconv", pb)


def test_ld_thconv():
    """the thin 32 -> 16 data gradient at 32 x 32 (of the 16 -> 32 convolution)."""
    pb = Problem("conv_dgrad", "bf16", 3, 16, 32, 32, 32, 3, 1, 1)
    demonstrated("thconv", (3, 16, 32, 32, 3, 1, 1), contract("thconv", pb, (8, 24), {}, dict(disable=L.K_THCONV)))
    poison_ldx("thconv", pb)


@pytest.mark.parametrize("case", [(3, 16, 32, 32, 1, 1, 0), (3, 32, 64, 32, 1, 2, 0)])
def test_ld_pconv(case):
    """the 1x1 shortcut forward (prologue only: the guard declines a bias, a residual and the statistics); (c) -- with the
    statistics -- is answered by the kernel behind it."""
    B, Cin, N, H, k, s, pd = case
    pb = Problem("conv", "bf16", B, Cin, N, H, H, k, s, pd, bias=False, res=False)
    demonstrated("pconv", case, contract("pconv", pb, (8, 24), {}, dict(disable=L.K_PCONV), stats=False))
    for pad in (8, 24):
        check("pconv/stats", pb, *pb.launch(0, pad, True))
    poison_ldx("pconv", pb)


@pytest.mark.parametrize("Cin", [64, 32])
def test_ld_dconv(Cin):
    """the data gradient of ConvTranspose2d(Cin, 16, 4, 2, 1) at 16 x 16 -> 32 x 32: a 4x4 stride-2 convolution 16 -> Cin."""
    pb = Problem("convT_dgrad", "bf16", 3, Cin, 16, 16, 16, 4, 2, 1)
    demonstrated("dconv", (3, Cin, 16, 16), contract("dconv", pb, (4, 8, 24), {}, dict(disable=L.K_TCONVR_EX)))
    poison_ldx("dconv", pb)


@pytest.mark.parametrize("name", ["convT_128_64", "convT_128_64_noepi", "last_decoder_layer", "dgrad_64_128", "dgrad_32_64"])
def test_ld_tconv(name):
    """tconv.hip: ConvTranspose2d(4, 2, 1) 128 -> 64 at 8 x 8 (prologue + statistics; bare), the last decoder layer 64 -> 16 at
    16 x 16 (prologue only: ldo % 8), and the EX forms -- the data gradients of the stride-2 3x3 convolutions 64 -> 128 / 32 -> 64."""
    off = dict(disable=L.K_TCONVR)
    if name == "convT_128_64":
        hits = contract("tconv", Problem("convT", "bf16", 3, 128, 64, 8, 8, 4, 2, 1, bias=False, res=False), (4, 8, 24), {}, off)
    elif name == "convT_128_64_noepi":
        hits = contract("tconv", Problem("convT", "bf16", 3, 128, 64, 8, 8, 4, 2, 1, pro=False, bias=False, res=False), (4, 8), {}, off, stats=False)
    elif name == "last_decoder_layer":
        pb = Problem("convT", "bf16", 3, 64, 16, 16, 16, 4, 2, 1, bias=False, res=False)
        hits = contract("tconv", pb, (8, 24), {}, off, stats=False)
        poison_ldx("tconv", pb)
    elif name == "dgrad_64_128":
        hits = contract("tconv", Problem("conv_dgrad", "bf16", 3, 64, 128, 16, 16, 3, 2, 1), (4, 8, 24), {}, off)
    else:
        hits = contract("tconv", Problem("conv_dgrad", "bf16", 3, 32, 64, 32, 32, 3, 2, 1), (4, 8, 24), {}, off)
    demonstrated("tconv", (name,), hits)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("persistent", [True, False])
def test_ld_halo(dt, persistent):
    """halop (persistent) and halo (one tile per block) under SV_OPT_HALO_ALL: the stride-2 3x3 forward with every fusion and
    ConvTranspose2d(4, 2, 1) 64 -> 16 at 16 x 16 with its statistics (four phases)."""
    base = L.K_TCONVR | (0 if persistent else L.K_HALOP)
    on, off = dict(halo_all=1, disable=base), dict(halo_all=1, disable=base | L.K_HALO | L.K_HALOP)
    family = "halop" if persistent else "halo"
    hits = contract(family, Problem("conv", dt, 3, 32, 64, 16, 16, 3, 2, 1), (4, 8, 24), on, off)
    hits += contract(family, Problem("convT", dt, 3, 64, 16, 16, 16, 4, 2, 1, bias=False, res=False, seed=2), (4, 8, 24), on, off)
    demonstrated(family, (dt,), hits)
    poison_ldx(family, Problem("conv", dt, 3, 32, 64, 16, 16, 3, 2, 1, seed=4), on)


GENERIC = [dict(disable=L.K_HALO | L.K_HALOP), dict(disable=L.K_HALO | L.K_HALOP, wide_min_blocks=1)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(5, 64, 128, 8, 3, 2, 1), (4, 32, 64, 16, 1, 2, 0), (37, 144, 1024, 1, 1, 1, 0)])
def test_ld_generic(dt, case):
    """The gather-GEMM (64 x MS-row tiles; with wide_min_blocks = 1 the 256-row tiles, and the LDS-DMA kernel on the data gradient)
    with padded ldo, padded (NaN-filled) ldx and both: against the reference only."""
    B, Cin, N, H, k, s, pd = case
    fwd = Problem("conv", dt, B, Cin, N, H, H, k, s, pd)
    bwd = Problem("conv_dgrad", dt, B, Cin, N, H, H, k, s, pd, seed=3)
    for opts in GENERIC:
        for pb in (fwd, bwd):
            for ldx_pad, ldo_pad in ((0, 8), (0, 24), (0, 4), (8, 0), (24, 0), (8, 24), (24, 8)):
                check("generic", pb, *pb.launch(ldx_pad, ldo_pad, True, opts))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_ld_groups(dt):
    """A batched launch of three groups: the group stride B * H * W * ld (common.h) with ld wider than the channel count --
    through the gather-GEMM with both leading dimensions padded, and through conv3x3p with a padded ldo (its guard requires
    ldx == Cin, conv3x3.hip conv3x3_covers)."""
    case = (4, 32, 32, 32, 3, 1, 1)
    B, Cin, N, H, k, s, pd = case
    fwd = Problem("conv", dt, B, Cin, N, H, H, k, s, pd, groups=3)
    bwd = Problem("conv_dgrad", dt, B, Cin, N, H, H, k, s, pd, groups=3, seed=3)
    for pb in (fwd, bwd):
        for opts in GENERIC:
            o = dict(opts, disable=opts["disable"] | L.K_CONV3X3)
            check("generic/groups", pb, *pb.launch(8, 24, True, o))
            check("generic/groups", pb, *pb.launch(24, 8, True, o))
        contract("conv3x3p/groups", pb, (8, 24), {}, dict(disable=L.K_CONV3X3P))       # (CITED: the shape of test_ld_conv3x3_persistent)


# ------------------------------------------------------------------------------------ 2. rectangular and odd-sized maps
RECT = [
    # B, Cin, N, H, W, k, stride, pad
    (3, 32, 64, 8, 16, 3, 1, 1),       # powers of two, rectangular: every square-only guard has to refuse
    (3, 32, 64, 16, 8, 3, 1, 1),       # the transpose: a swapped Hin / Win
    (2, 64, 64, 12, 12, 3, 1, 1),      # square, not a power of two (hwsh = -1)
    (5, 32, 32, 7, 7, 3, 1, 1),        # B * Hq * Wq = 245: not a multiple of 128
    (3, 16, 32, 6, 10, 3, 1, 1),
    (2, 64, 128, 12, 20, 3, 2, 1),     # a four-phase data gradient
    (3, 32, 64, 6, 10, 1, 2, 0),       # phases without taps
    (2, 16, 32, 1, 9, 3, 1, 1),        # pruned to three taps
]


def rect_problems(dt, case, groups=1):
    B, Cin, N, H, W, k, s, pd = case
    return (Problem("conv", dt, B, Cin, N, H, W, k, s, pd, groups=groups),
            Problem("conv_dgrad", dt, B, Cin, N, H, W, k, s, pd, groups=groups, seed=3))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", RECT)
def test_rect_forward_and_dgrad(dt, case):
    """Forward with prologue, bias, residual and statistics, data gradient with the `ex` epilogue, default dispatch."""
    fwd, bwd = rect_problems(dt, case)
    if case[3:5] == (1, 9):
        assert fwd.geom().phase[0].ntap == 3
    check("rect", fwd, *fwd.launch())
    check("rect", bwd, *bwd.launch())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rect_wide_tiles(dt):
    """the 256-row (MS = 4) and LDS-DMA tiles of the gather-GEMM on an odd map (wide_min_blocks = 1)."""
    fwd, bwd = rect_problems(dt, (4, 160, 160, 6, 10, 3, 1, 1))
    check("rect/wide", fwd, *fwd.launch(opts=dict(wide_min_blocks=1)))
    check("rect/wide", bwd, *bwd.launch(opts=dict(wide_min_blocks=1)))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rect_groups(dt):
    fwd, bwd = rect_problems(dt, (3, 16, 32, 6, 10, 3, 1, 1), groups=2)
    check("rect/groups", fwd, *fwd.launch())
    check("rect/groups", bwd, *bwd.launch())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rect_sparse_out(dt):
    """The data gradient of a stride-2 1x1 convolution on a 6 x 10 map with sparse_out = 1: the three phases without taps are
    skipped -- their positions keep the sentinel -- and the even positions and the sums are those of the dense result."""
    pb = rect_problems(dt, (3, 32, 64, 6, 10, 1, 2, 0))[1]
    out, sums, info = pb.launch(sparse_out=1)
    n = pb.gout
    even = torch.zeros(6, 10, dtype=torch.bool)
    even[0::2, 0::2] = True
    assert bool((out[:, ~even] == SENTINEL).all()), "a skipped position was written"
    e = rel(out[:, even][..., :n], pb.y[:, even])
    report("rect/sparse", dt, "out", e)
    assert e < DT[dt][2]
    assert float(pb.y[:, ~even].abs().max()) == 0.0               # (the reference is zero there: the sums are unchanged)
    for half in (slice(0, n), slice(n, 2 * n)):
        e = rel(sums[0, half], pb.sums[0, half])
        report("rect/sparse", dt, "sums", e)
        assert e < sums_tol(dt)
    assert bool((info["lo"] == SENTINEL).all()) and bool((info["hi"] == SENTINEL).all())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,H,W", [(3, 3, 5), (4, 1, 4)])
def test_rect_convT(dt, B, H, W):
    """ConvTranspose2d(64, 16, 4, 2, 1) on 3 x 5 and 1 x 4 maps with its data gradient, the 4x4 stride-2 convolution at 2H x 2W."""
    fwd = Problem("convT", dt, B, 64, 16, H, W, 4, 2, 1, bias=False, res=False)
    bwd = Problem("convT_dgrad", dt, B, 64, 16, H, W, 4, 2, 1, seed=3)
    check("rect/convT", fwd, *fwd.launch())
    check("rect/convT", bwd, *bwd.launch())


def run_wgrad(g, dt, x, dy, pro, use_tr, groups=1, workspace=(False, True)):
    """sv_wgrad_ex, one call per entry of `workspace` (with / without the slab workspace) accumulating into one gradient;
    -> dw [N][T][Cin] / len(workspace)"""
    code, tdt, _ = DT[dt]
    d = dev()
    xd, dyd = x.to(d, tdt).contiguous(), dy.to(d, tdt).contiguous()
    sc, sh = pro[0].to(d).contiguous(), pro[1].to(d).contiguous()
    dw = torch.zeros(g.N, g.T_orig, g.Cin, device=d)
    ws = torch.full((4 * 1024 * 1024,), float("nan"), device=d)      # workspace contents are irrelevant on entry
    for with_ws in workspace:
        a = L.SvWgradArgs()
        a.x, a.dy, a.dw = xd.data_ptr(), dyd.data_ptr(), dw.data_ptr()
        a.pro_scale, a.pro_shift, a.pro_slope = sc.data_ptr(), sh.data_ptr(), pro[2]
        a.splits, a.use_tr, a.groups = 0, use_tr, groups
        if with_ws:
            a.ws, a.ws_elems = ws.data_ptr(), ws.numel()
        L.call("sv_wgrad_ex", C.byref(g), code, C.byref(a), st())
    torch.cuda.synchronize()
    return dw.cpu() / len(workspace)


def wgrad_problem(dt, case, groups=1, transposed=False):
    """-> geometry, x, dy (NHWC), prologue, reference dW in the master layout [N][T][Cin] (float64)"""
    B, Cin, N, H, W, k, s, pd = case
    torch.manual_seed(5)
    GB = groups * B
    x = bq(torch.randn(GB, Cin, H, W), dt)
    scale, shift = torch.rand(groups, Cin) + 0.5, torch.randn(groups, Cin) * 0.3
    gi = torch.arange(GB) // B
    a = bq(F.leaky_relu(x * scale[gi][:, :, None, None] + shift[gi][:, :, None, None], SLOPE), dt).to(F64)
    if transposed:
        dy = bq(torch.randn(GB, N, 2 * H, 2 * W), dt)
        w0 = torch.zeros(Cin, N, 4, 4, dtype=F64, requires_grad=True)
        F.conv_transpose2d(a, w0, None, 2, 1).backward(dy.to(F64))
        ref = w0.grad.permute(1, 2, 3, 0).reshape(N, 16, Cin)
        g = G.convT_like(B, H, W, Cin, N, 4, 2, 1)
    else:
        Ho, Wo = (H + 2 * pd - k) // s + 1, (W + 2 * pd - k) // s + 1
        dy = bq(torch.randn(GB, N, Ho, Wo), dt)
        ref = torch.nn.grad.conv2d_weight(a, (N, Cin, k, k), dy.to(F64), s, pd).permute(0, 2, 3, 1).reshape(N, k * k, Cin)
        g = G.conv_like(B, H, W, Cin, N, k, s, pd)
    return g, nhwc(x), nhwc(dy), (scale, shift, SLOPE), ref


WG_RECT = RECT + [(4, 160, 160, 6, 10, 3, 1, 1)]


@pytest.mark.parametrize("dt,use_tr", [("f32", 0), ("bf16", 0), ("bf16", 1)])
@pytest.mark.parametrize("case", WG_RECT)
def test_rect_wgrad(dt, use_tr, case):
    """The generic weight gradient (FAST = false off the powers of two), two accumulating calls -- without and with a workspace."""
    g, x, dy, pro, ref = wgrad_problem(dt, case)
    with L.options(wide_min_blocks=1 if case[1] == 160 else None):
        got = run_wgrad(g, dt, x, dy, pro, use_tr)
    e = rel(got, ref)
    report("rect/wgrad", dt, "dw", e)
    assert e < DT[dt][2], e


@pytest.mark.parametrize("dt,use_tr", [("f32", 0), ("bf16", 1)])
@pytest.mark.parametrize("case,transposed", [((3, 16, 32, 6, 10, 3, 1, 1), False), ((4, 160, 160, 6, 10, 3, 1, 1), False),
                                             ((3, 64, 16, 3, 5, 4, 2, 1), True), ((4, 64, 16, 1, 4, 4, 2, 1), True)])
def test_rect_wgrad_groups_and_convT(dt, use_tr, case, transposed):
    """Two groups (the gradient of the shared weights sums over them; 160 -> 160 with wide_min_blocks = 1: the cooperative wide
    kernel's FAST = false instantiation in bf16) and the ConvTranspose2d(4, 2, 1) weight gradient on 3 x 5 / 1 x 4 maps."""
    g, x, dy, pro, ref = wgrad_problem(dt, case, groups=2, transposed=transposed)
    with L.options(wide_min_blocks=1 if case[1] == 160 else None):
        got = run_wgrad(g, dt, x, dy, pro, use_tr, groups=2)
    e = rel(got, ref)
    report("rect/wgrad", dt, "dw", e)
    assert e < DT[dt][2], e


@pytest.mark.parametrize("dt,use_tr", [("f32", 0), ("bf16", 1)])
def test_rect_wgrad_deterministic(dt, use_tr):
    """SV_OPT_DETERMINISTIC on a 7 x 7 map with a workspace -- 588 rows, two M ranges: the slab path of wgrad_generic_try (one
    slab per range, reduced in a fixed order).  Two runs agree bit for bit and match the reference."""
    g, x, dy, pro, ref = wgrad_problem(dt, (12, 32, 32, 7, 7, 3, 1, 1))
    with L.options(deterministic=1):
        a = run_wgrad(g, dt, x, dy, pro, use_tr, workspace=(True,))
        b = run_wgrad(g, dt, x, dy, pro, use_tr, workspace=(True,))
    assert torch.equal(a, b)
    e = rel(a, ref)
    report("rect/wgrad/det", dt, "dw", e)
    assert e < DT[dt][2], e


@pytest.mark.parametrize("what", ["rect", "ldo"])
def test_bwd3x3_refuses_off_model_geometry(what):
    """sv_bwd3x3 covers square 8 / 16 / 32 maps with dense leading dimensions: an 8 x 16 map and ldo = N + 8 are refused by its own
    shape check (SV_E_SHAPE) and nothing is launched -- dw, out and bsums keep their contents."""
    d = dev()
    B, Cc = 4, 32
    g = G.convT_like(B, 8, 16, Cc, Cc, 3, 1, 1) if what == "rect" else G.convT_like(B, 16, 16, Cc, Cc, 3, 1, 1, ldo=Cc + 8)
    rows = B * g.Hout * g.Wout
    dy = torch.zeros(rows * g.ldx, dtype=torch.bfloat16, device=d)
    x = torch.zeros(rows * g.ldo, dtype=torch.bfloat16, device=d)
    w = torch.zeros(9 * Cc * Cc, dtype=torch.bfloat16, device=d)
    out = torch.full((rows * g.ldo,), SENTINEL, dtype=torch.bfloat16, device=d)
    dw = torch.full((Cc * 9 * Cc,), SENTINEL, device=d)
    bsums = torch.full((4 * 2 * Cc,), SENTINEL, dtype=ACC, device=d)
    ws = torch.zeros(256 * 9 * Cc * Cc, device=d)
    vec = torch.ones(Cc, device=d)
    a = L.SvBwd3x3Args()
    a.dy, a.x, a.w, a.out, a.dw, a.bsums = dy.data_ptr(), x.data_ptr(), w.data_ptr(), out.data_ptr(), dw.data_ptr(), bsums.data_ptr()
    a.x_scale = a.x_shift = a.x_mean = a.x_rstd = vec.data_ptr()
    a.x_slope, a.replicas, a.groups, a.ws, a.ws_elems = SLOPE, 4, 1, ws.data_ptr(), ws.numel()
    rc = L.lib().sv_bwd3x3(C.byref(g), L.SV_BF16, C.byref(a), st())
    assert rc == -2, rc                                                     # SV_E_SHAPE
    assert b"sv_bwd3x3: stride-1 3x3 layers" in L.lib().sv_last_error()
    torch.cuda.synchronize()
    assert bool((out.float() == SENTINEL).all()) and bool((dw == SENTINEL).all()) and bool((bsums == SENTINEL).all())
