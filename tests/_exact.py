"""Exact integer parity for the convolution family: operands, float64 references, the conditions under which a correct kernel
owes EQUALITY, and the comparator.  Pure torch on the CPU; importable without a GPU (tests/test_conv_exact_cpu.py proves the case
tables, tests/test_conv_exact_gpu.py runs them).

Why equality is owed.  sv_igemm, sv_wgrad_ex and sv_bwd3x3 multiply storage-type operands and accumulate in fp32.  With small
integers (and halves) as operands every product and every partial sum is exactly representable, so the order of the additions --
split-K, slabs, float atomics, replicas -- cannot matter, and a bf16 output that is an integer of magnitude <= 256 (a half-integer
<= 128) is stored without rounding.  `preconditions` asserts exactly that on the float64 reference, case by case.

Construction (one seeded generator per case):
  x, dy, the raw `ex` tensor   integers in [-2, 2] ({-1, 0, 1} for `small` cases)
  prologue / ex coefficients   scale 2, shift even in [-4, 4] ([-2, 2] for `small`), slope 0.5: u = 2 x + shift is an even integer,
                               the activated value u or u / 2 is an integer, the derivative factor 1 or 1 / 2 is exact, and u == 0 is
                               frequent -- the convention `u > 0 ? 1 : slope` (common.h act_grad) is pinned at u == 0
  ex_mean, ex_rstd             integers in [-1, 1]; {0.5, 1, 2}
  bias, residual               integers in [-3, 3] / [-4, 4]
  weights                      +-1 (balanced per row) on the mask  (j mod M == n mod M)  of the [N][taps * Cin] matrix, M chosen so
                               that the reduction the case tests has about 32 terms (`small`: 16 forward, 48 in a data gradient,
                               whose terms are {-1, 0, 1} and cancel to zero more often -- (e)); a stride-2 data gradient counts
                               the terms of its one-tap phase (12 / 24 there, four times as many in the four-tap phase),
                               ConvTranspose2d(4, 2, 1) the four taps an output pixel sees (one on maps of up to 4 x 4)
  groups                       every group draws its own shifts; the mean / rstd patterns are rotated by one channel per group
`small` cases are the large batches (B >= 70 on a persistent kernel, conv3x3m's 256-block grid): their channel sums run over 10^5
elements and would leave the 2^24 window with the wider range."""
import dataclasses
import functools

import torch
import torch.nn.functional as F

from shot_vae_amd import _lib as L

F64 = torch.float64
SLOPE = 0.5
DW0 = 3.0            # what a weight gradient starts from (it accumulates: got == DW0 + calls * reference)
LIMIT = float(2 ** 24)


@dataclasses.dataclass(frozen=True)
class Case:
    """One layer Cin -> N on H x H maps (H: the LAYER's input map) and one form of it.
    kind: conv / convT (forward), conv_dgrad / convT_dgrad (data gradient; `ex`: with the activation-backward epilogue),
    wgrad / wgradT (weight gradient of Conv2d / ConvTranspose2d(4, 2, 1)), bwd (sv_bwd3x3; form 0 / 1 / 2)."""
    kind: str
    B: int
    Cin: int
    N: int
    H: int
    k: int = 3
    stride: int = 1
    pad: int = 1
    groups: int = 1
    pro: bool = True
    bias: bool = True
    res: bool = True
    stats: bool = True
    ex: bool = True
    small: bool = False
    form: int = 0
    seed: int = 1

    @property
    def Ho(self):
        return 2 * self.H if self.kind.startswith(("convT", "wgradT")) else (self.H + 2 * self.pad - self.k) // self.stride + 1


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _grid(*ts):
    """the coarsest power of two (down to 2^-4) that every value of ts is a multiple of"""
    g = 1.0
    while g > 2.0 ** -4 and any(bool((t / g != (t / g).round()).any()) for t in ts):
        g /= 2
    assert all(bool((t / g == (t / g).round()).all()) for t in ts), "values off the 2^-4 grid"
    return g


def _ints(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F64)


def _per(v, B):
    """[groups][C] -> [groups * B, C, 1, 1]"""
    return v.repeat_interleave(B, 0)[:, :, None, None]


def _pattern(values, groups, C, offset=0):
    """[groups][C]: `values` cycled over the channels, rotated by one per group (deterministic: every value occurs)"""
    idx = (torch.arange(C)[None, :] + torch.arange(groups)[:, None] + offset) % len(values)
    return torch.tensor(values, dtype=F64)[idx]


def mask_period(c):
    T = c.k * c.k
    K = T * c.Cin
    nnz = 16 if c.small else 32                # forward: terms of magnitude up to 8 (4 for `small`)
    dnz = 48 if c.small else 32                # data gradient: terms of magnitude up to 2 (1 for `small`)
    if c.kind in ("conv", "wgrad", "wgradT"):
        M = -(-K // nnz)
    elif c.kind == "convT":                    # an output pixel sees four taps; on maps of up to 4 x 4 the corner pixels see one
        M = max(1, c.Cin // 12) if c.H <= 4 else -(-K // (4 * nnz))
    elif c.kind == "convT_dgrad":              # sixteen taps; on small maps the corner pixels see four (1 x 1) or nine of them
        M = -(-((4 if c.H == 1 else 9 if c.H <= 4 else T) * c.N) // dnz)
    elif c.stride == 2 and c.k == 3:           # conv_dgrad, four phases of 1 / 2 / 2 / 4 taps: count the one-tap phase
        M = max(1, c.N // (24 if c.small else 12))
    else:                                      # conv_dgrad / bwd, stride 1
        M = -(-(T * c.N) // dnz)
    return max(1, min(M, c.N, K))


def weights(c, gen):
    """master [N][taps][Cin]: +-1 where (j mod M) == (n mod M), j the column of the [N][taps * Cin] matrix.  The signs of a row are
    a random half +1, half -1: an activated input has a non-zero mean, and a row whose signs do not cancel gives its output channel
    a mean that the sum of squares (c) then pays for."""
    T = c.k * c.k
    K, M = T * c.Cin, mask_period(c)
    mask = (torch.arange(K)[None, :] % M) == (torch.arange(c.N)[:, None] % M)
    keys = torch.rand(c.N, K, generator=gen, dtype=F64)
    keys[~mask] = 2.0                                    # the non-zeros of a row get the ranks 0 .. count - 1 in random order
    rank = keys.argsort(1).argsort(1)
    sign = torch.where(rank % 2 == 0, 1.0, -1.0).to(F64)
    return (mask.to(F64) * sign).view(c.N, T, c.Cin)


def torch_weight(c, master):
    """OIHW for a Conv2d, IOHW for a ConvTranspose2d"""
    m = master.view(c.N, c.k, c.k, c.Cin)
    return (m.permute(3, 0, 1, 2) if c.kind.startswith(("convT", "wgradT")) else m.permute(0, 3, 1, 2)).contiguous()


def act(u):
    return torch.where(u > 0, u, u * SLOPE)


def act_grad(u):
    """common.h act_grad: u > 0 ? 1 : slope -- the slope AT u == 0"""
    return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, SLOPE))


def _coeffs(c, C, gen):
    """scale, shift [groups][C] of a prologue / ex epilogue: u = 2 x + shift is even, so u / 2 is an integer; every shift of the
    set puts u == 0 at one value of x (a fifth of the elements; a third for `small`)"""
    scale = torch.full((c.groups, C), 2.0, dtype=F64)
    values = torch.tensor((0, 2, -2) if c.small else (0, 2, -2, 4, -4), dtype=F64)
    shift = values[torch.randint(0, len(values), (c.groups, C), generator=gen)]
    return scale, shift


class Built:
    """operands, reference outputs and the bookkeeping `preconditions` reads"""

    def __init__(self, case):
        self.case = case
        self.operands = {}      # name -> tensor that is stored in the storage type
        self.outputs = {}       # name -> reference tensor that the kernel stores in the storage type
        self.accum = {}         # name -> (sum of |terms| (tensor or bound), grid)
        self.us = []            # pre-activation values whose sign decides something
        self.master = None


def _fwd_conv(c, a, w, bias):
    return F.conv2d(a, w, bias, c.stride, c.pad) if c.kind == "conv" else F.conv_transpose2d(a, w, bias, 2, 1)


def _dgrad(c, dy, w):
    if c.kind == "convT_dgrad":
        return F.conv2d(dy, w, None, 2, 1)
    Ho = c.Ho
    op = c.H - ((Ho - 1) * c.stride - 2 * c.pad + c.k)
    return F.conv_transpose2d(dy, w, None, c.stride, c.pad, output_padding=op)


def _group_sums(c, first, second):
    """[groups][2 C] channel sums of two [groups * B, C, H, W] tensors"""
    f = first.view(c.groups, c.B, *first.shape[1:]).sum((1, 3, 4))
    s = second.view(c.groups, c.B, *second.shape[1:]).sum((1, 3, 4))
    return torch.cat([f, s], 1)


@functools.lru_cache(maxsize=4)
def build(c):
    gen = torch.Generator().manual_seed(1000 + c.seed)
    r = 1 if c.small else 2
    GB = c.groups * c.B
    b = Built(c)
    if c.kind not in ("wgrad", "wgradT"):
        b.master = weights(c, gen)
        b.operands["w"] = b.master
        w = torch_weight(c, b.master)
    if c.kind in ("conv", "convT"):
        b.x = _ints(gen, -r, r, (GB, c.Cin, c.H, c.H))
        b.operands["x"] = b.x
        a = b.x
        b.pro = None
        if c.pro:
            scale, shift = _coeffs(c, c.Cin, gen)
            b.pro = (scale, shift, SLOPE)
            u = b.x * _per(scale, c.B) + _per(shift, c.B)
            b.us.append(u)
            a = act(u)
            b.operands["act(x)"] = a
        b.bias = _ints(gen, -3, 3, (c.N,)) if c.bias else None
        y = _fwd_conv(c, a, w, b.bias)
        b.res = None
        if c.res:
            b.res = _ints(gen, -4, 4, tuple(y.shape))
            b.operands["residual"] = b.res
            y = y + b.res
        b.y = y
        b.outputs["out"] = y
        rows = b.master.view(c.N, -1).abs().sum(1).max()
        b.accum["out"] = (rows * a.abs().max() + 3 + 4, _grid(a))
        if c.stats:
            b.sums = _group_sums(c, y, y * y)
            b.accum["stats.sum"] = (_group_sums(c, y.abs(), y * y), _grid(y) ** 2)
    elif c.kind in ("conv_dgrad", "convT_dgrad"):
        Ho = c.Ho
        b.dy = _ints(gen, -r, r, (GB, c.N, Ho, Ho))
        b.operands["dy"] = b.dy
        da = _dgrad(c, b.dy, w)
        cols = b.master.abs().sum((0, 1)).max()
        b.accum["out"] = (cols * r, 1.0)
        b.exd = None
        y = da
        if c.ex:
            xraw = _ints(gen, -r, r, (GB, c.Cin, c.H, c.H))
            b.operands["ex"] = xraw
            scale, shift = _coeffs(c, c.Cin, gen)
            mean = _pattern((0, 1, -1), c.groups, c.Cin, 1)
            rstd = _pattern((1.0, 0.5, 2.0, 1.0), c.groups, c.Cin, 2)
            b.exd = dict(x=xraw, scale=scale, shift=shift, mean=mean, rstd=rstd, slope=SLOPE)
            u = xraw * _per(scale, c.B) + _per(shift, c.B)
            b.us.append(u)
            y = da * act_grad(u)
            xh = (xraw - _per(mean, c.B)) * _per(rstd, c.B)
            b.sums = _group_sums(c, y, y * xh)
            b.accum["bsums"] = (_group_sums(c, y.abs(), (y * xh).abs()), _grid(y) * _grid(xh))
        b.y = y
        b.outputs["out"] = y
    elif c.kind in ("wgrad", "wgradT"):
        Ho = c.Ho
        b.x = _ints(gen, -r, r, (GB, c.Cin, c.H, c.H))
        b.dy = _ints(gen, -r, r, (GB, c.N, Ho, Ho))
        b.operands.update(x=b.x, dy=b.dy)
        a = b.x
        b.pro = None
        if c.pro:
            scale, shift = _coeffs(c, c.Cin, gen)
            b.pro = (scale, shift, SLOPE)
            u = b.x * _per(scale, c.B) + _per(shift, c.B)
            b.us.append(u)
            a = act(u)
            b.operands["act(x)"] = a
        b.dw = wgrad_reference(c, a, b.dy)
        # every output position contributes one term |a| * |dy| to a weight: a bound on the sum of their magnitudes
        b.accum["dw"] = (GB * Ho * Ho * a.abs().max() * r, _grid(a))
        b.y = b.dw
    elif c.kind == "bwd":
        assert c.k == 3 and c.stride == 1 and c.Cin == c.N
        Cc, H = c.Cin, c.H
        b.dy = _ints(gen, -r, r, (GB, Cc, H, H))
        b.operands["dy"] = b.dy
        eff = b.dy
        b.coef = b.dy2 = b.dy3 = None
        if c.form >= 1:
            b.dy2 = _ints(gen, -r, r, (GB, Cc, H, H))
            b.operands["dy2"] = b.dy2
            b.coef = (_pattern((1, 2), c.groups, Cc), _pattern((-1, 0, 1), c.groups, Cc, 1), _pattern((0, 1, -1, 0, 2, -2), c.groups, Cc, 2))
            eff = b.dy * _per(b.coef[0], c.B) + (b.dy2 * _per(b.coef[1], c.B) + _per(b.coef[2], c.B))
        if c.form == 2:
            b.dy3 = _ints(gen, -1, 1, (GB, Cc, H, H))
            b.operands["dy3"] = b.dy3
            eff = eff + b.dy3
            b.outputs["dy_out"] = eff
        b.eff = eff
        b.operands["dy formed"] = eff
        xraw = _ints(gen, -r, r, (GB, Cc, H, H))
        b.operands["x"] = xraw
        scale, shift = _coeffs(c, Cc, gen)
        mean = _pattern((0, 1, -1), c.groups, Cc, 1)
        rstd = _pattern((1.0, 0.5, 2.0, 1.0), c.groups, Cc, 2)
        b.exd = dict(x=xraw, scale=scale, shift=shift, mean=mean, rstd=rstd, slope=SLOPE)
        u = xraw * _per(scale, c.B) + _per(shift, c.B)
        b.us.append(u)
        a = act(u)
        b.operands["act(x)"] = a
        da = F.conv_transpose2d(eff, w, None, 1, 1)
        y = da * act_grad(u)
        xh = (xraw - _per(mean, c.B)) * _per(rstd, c.B)
        b.y = y
        b.outputs["out"] = y
        b.sums = _group_sums(c, y, y * xh)
        b.dw = torch.nn.grad.conv2d_weight(a, (Cc, Cc, 3, 3), eff, 1, 1).permute(0, 2, 3, 1).reshape(Cc, 9, Cc)
        cols = b.master.abs().sum((0, 1)).max()
        b.accum["out"] = (cols * eff.abs().max(), 1.0)
        b.accum["bsums"] = (_group_sums(c, y.abs(), (y * xh).abs()), _grid(y) * _grid(xh))
        b.accum["dw"] = (GB * H * H * a.abs().max() * eff.abs().max(), _grid(a))
    else:
        raise ValueError(c.kind)
    return b


def wgrad_reference(c, a, dy):
    """dW in the master layout [N][taps][Cin], summed over the groups (they share the weights)"""
    if c.kind == "wgradT":
        w0 = torch.zeros(c.Cin, c.N, 4, 4, dtype=F64, requires_grad=True)
        F.conv_transpose2d(a, w0, None, 2, 1).backward(dy)
        return w0.grad.permute(1, 2, 3, 0).reshape(c.N, 16, c.Cin)
    return torch.nn.grad.conv2d_weight(a, (c.N, c.Cin, c.k, c.k), dy, c.stride, c.pad).permute(0, 2, 3, 1).reshape(c.N, c.k * c.k, c.Cin)


def preconditions(c, calls=2):
    """The conditions under which a correct kernel owes equality, asserted on the reference alone ((a) - (f) of the module's case
    for exactness).  `calls`: how often a weight gradient accumulates into DW0."""
    b = build(c)
    # (a) every operand, and the activated prologue output, is its own bf16 rounding
    for name, t in b.operands.items():
        assert torch.equal(t, bf16(t)), (c, "(a)", name)
    # (b) every bf16 output of the reference is its own bf16 rounding
    for name, t in b.outputs.items():
        assert torch.equal(t, bf16(t)), (c, "(b)", name, float(t.abs().max()))
    # (c) every accumulated quantity: the sum of the magnitudes of its terms stays below 2^24 units of its grid
    for name, (total, grid) in b.accum.items():
        total = float(torch.as_tensor(total).max())
        if name == "dw":
            total = DW0 + calls * total
        assert total / grid < LIMIT, (c, "(c)", name, total, grid)
    if b.master is not None:
        # (d) every row and every column of the weight matrix has a non-zero
        m = b.master.view(c.N, -1)
        assert bool((m.abs().sum(1) > 0).all()) and bool((m.abs().sum(0) > 0).all()), (c, "(d)")
    # (e) at least 90 % of the output elements are non-zero
    nz = float((b.y != 0).to(F64).mean())
    assert nz >= 0.9, (c, "(e)", nz)
    # (f) u == 0, u > 0 and u < 0 each make up at least 5 % of the elements
    for u in b.us:
        for what, frac in (("== 0", (u == 0)), ("> 0", (u > 0)), ("< 0", (u < 0))):
            f = float(frac.to(F64).mean())
            assert f >= 0.05, (c, "(f)", what, f)
    return b


def assert_equal(got, want, what):
    """got == want element for element (so -0.0 equals 0.0); on failure: how many differ, the first ten as (index, got, want), and for
    4-D outputs [image, row, column, channel] the distinct (row, column) pairs and channels among the mismatches"""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape, (what, "shape", tuple(got.shape), tuple(want.shape))
    g, w = got.to(F64), want.to(F64)
    bad = ~(g == w)                           # (NaN differs from everything)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()
    lines = ["%s: %d of %d elements differ" % (what, n, bad.numel())]
    for i in idx[:10]:
        t = tuple(int(v) for v in i)
        lines.append("  %s got %r want %r" % (t, float(g[t]), float(w[t])))
    if got.dim() == 4:
        pos = sorted({(int(i[1]), int(i[2])) for i in idx})
        ch = sorted({int(i[3]) for i in idx})
        lines.append("  (row, column): %d distinct %s%s" % (len(pos), pos[:16], " ..." if len(pos) > 16 else ""))
        lines.append("  channels: %d distinct %s%s" % (len(ch), ch[:32], " ..." if len(ch) > 32 else ""))
    raise AssertionError("\n".join(lines))


# --------------------------------------------------------------------------------------------------------- the GPU case tables
HALO = L.K_HALO | L.K_HALOP
FULL = dict(pro=True, bias=True, res=True, stats=True)
PRO_STATS = dict(pro=True, bias=False, res=False, stats=True)
PRO_ONLY = dict(pro=True, bias=False, res=False, stats=False)
BARE_STATS = dict(pro=False, bias=False, res=False, stats=True)


def _ig(name, label, dt, case, **opts):
    return (name, label, dt, case, opts)


def _pair(name, labels, dt, dims, fwd_flags=FULL, groups=1, small=False, **opts):
    """the forward and the data gradient (ex epilogue) of one Conv2d layer under the same options"""
    B, Cin, N, H, k, s, p = dims
    out = []
    if labels[0]:
        out.append(_ig(name + "/fwd", labels[0], dt, Case("conv", B, Cin, N, H, k, s, p, groups=groups, small=small, **fwd_flags), **opts))
    if labels[1]:
        out.append(_ig(name + "/dgrad", labels[1], dt, Case("conv_dgrad", B, Cin, N, H, k, s, p, groups=groups, small=small, seed=3), **opts))
    return out


GEN, DMA = "sv_igemm", "sv_igemm(dma)"
C3, C3P, C3M, C3W, C3X = ("sv_igemm(conv3x3%s)" % s for s in ("", "p", "m", "w", "x"))
HAL, HALP, SCONV, PCONV, THCONV = ("sv_igemm(%s)" % s for s in ("halo", "halop", "sconv", "pconv", "thconv"))
TCONVR, TCONVX, DCONV, PIXEL = ("sv_igemm(%s)" % s for s in ("tconvr", "tconvx16", "dconv", "pixel"))

IGEMM = []
# the generic gather-GEMM: 32-channel tiles with a k tail (K = 16), fp32 and bf16; the 256-row tiles (ragged: 320 rows); a plain GEMM
# with a ragged batch and K = 144; the data gradients with the LDS-DMA kernel on and off
for _dt in ("f32", "bf16"):
    IGEMM += _pair("generic/1x1/" + _dt, (GEN, GEN), _dt, (4, 16, 32, 8, 1, 1, 0), disable=L.K_PCONV | HALO)
    IGEMM += _pair("generic/3x3s2/" + _dt, (GEN, GEN), _dt, (3, 32, 64, 16, 3, 2, 1), disable=L.K_SCONV | L.K_TCONVR | HALO | L.K_IGEMM_DMA)
    IGEMM += [_ig("generic/gemm/" + _dt, GEN, _dt, Case("conv", 37, 144, 1024, 1, 1, 1, 0, pro=False, res=False))]
IGEMM += _pair("generic/256rows", (GEN, None), "bf16", (5, 64, 128, 16, 3, 2, 1), wide_min_blocks=1, disable=HALO | L.K_TCONVR)
IGEMM += _pair("generic/256rows/nodma", (None, GEN), "bf16", (3, 320, 640, 16, 3, 2, 1), wide_min_blocks=1, disable=HALO | L.K_IGEMM_DMA)
IGEMM += _pair("generic/160", (GEN, None), "bf16", (7, 16, 160, 32, 1, 1, 0), wide_min_blocks=1, disable=L.K_PCONV | HALO)
IGEMM += _pair("generic/groups", (GEN, GEN), "bf16", (4, 16, 32, 8, 1, 1, 0), groups=3, disable=L.K_PCONV | HALO)
IGEMM += _pair("dma/wide", (None, DMA), "bf16", (3, 320, 640, 16, 3, 2, 1), wide_min_blocks=1, disable=HALO)
IGEMM += _pair("dma/128", (None, DMA), "bf16", (6, 128, 128, 8, 3, 1, 1), wide_min_blocks=1, disable=HALO | L.K_CONV3X3)
IGEMM += [_ig("dma/128/fwd-no-prologue", DMA, "bf16", Case("conv", 6, 128, 128, 8, 3, 1, 1, pro=False), wide_min_blocks=1, disable=HALO | L.K_CONV3X3)]
IGEMM += _pair("dma/groups", (None, DMA), "bf16", (6, 128, 128, 8, 3, 1, 1), groups=3, wide_min_blocks=1, disable=HALO | L.K_CONV3X3)
# conv3x3.hip: one tile per block (fp32 and bf16; 160 channels by default dispatch), the persistent kernel, the multi-tile kernel
for _dt in ("f32", "bf16"):
    IGEMM += _pair("conv3x3/" + _dt, (C3, C3), _dt, (2, 32, 96, 16, 3, 1, 1), disable=L.K_CONV3X3P)
    IGEMM += _pair("conv3x3p/" + _dt, (C3P, C3P), _dt, (4, 32, 32, 32, 3, 1, 1))
IGEMM += _pair("conv3x3/160", (C3, C3), "bf16", (2, 160, 160, 8, 3, 1, 1))
IGEMM += _pair("conv3x3/groups", (C3, C3), "bf16", (2, 32, 96, 16, 3, 1, 1), groups=3, disable=L.K_CONV3X3P)
IGEMM += _pair("conv3x3p/64", (C3P, C3P), "bf16", (4, 64, 64, 16, 3, 1, 1))
IGEMM += _pair("conv3x3p/groups", (C3P, C3P), "bf16", (4, 32, 32, 32, 3, 1, 1), groups=3)
IGEMM += _pair("conv3x3p/budget", (C3P, C3P), "bf16", (6, 32, 32, 32, 3, 1, 1), persistent_blocks=8)
IGEMM += _pair("conv3x3m", (C3M, C3M), "bf16", (32, 160, 160, 32, 3, 1, 1), small=True)
IGEMM += _pair("conv3x3m/groups", (C3M, C3M), "bf16", (11, 160, 160, 32, 3, 1, 1), groups=3, small=True)
# conv3x3w.hip / conv3x3x.hip: 160- and 128-channel tiles, one and several channel tiles, the run-time-flag and the compile-time binaries
for _name, _lab, _off in (("conv3x3w", C3W, L.K_CONV3X3X), ("conv3x3x", C3X, 0)):
    IGEMM += _pair(_name + "/160x8", (_lab, _lab), "bf16", (4, 160, 160, 8, 3, 1, 1), wide_min_blocks=1, disable=_off)
    IGEMM += _pair(_name + "/320x32", (_lab, _lab), "bf16", (3, 160, 320, 32, 3, 1, 1), wide_min_blocks=1, disable=_off)
    IGEMM += _pair(_name + "/nobias", (_lab, None), "bf16", (4, 160, 160, 8, 3, 1, 1), fwd_flags=dict(pro=True, bias=False, res=True, stats=True),
                   wide_min_blocks=1, disable=_off)
    IGEMM += _pair(_name + "/groups", (_lab, _lab), "bf16", (4, 160, 160, 8, 3, 1, 1), groups=3, wide_min_blocks=1, disable=_off)
IGEMM += _pair("conv3x3w/128", (C3W, C3W), "bf16", (8, 128, 128, 8, 3, 1, 1), wide_min_blocks=1)
IGEMM += _pair("conv3x3x/640", (C3X, C3X), "bf16", (4, 640, 640, 8, 3, 1, 1), wide_min_blocks=1)
IGEMM += _pair("conv3x3x/items", (C3X, C3), "bf16", (70, 96, 320, 16, 3, 1, 1), small=True, wide_min_blocks=1)
# halo.hip under SV_OPT_HALO_ALL: the stride-2 3x3 forward with every fusion, ConvTranspose2d(4, 2, 1) 64 -> 16 with its statistics;
# by default dispatch the thin-output data gradient 160 -> 16
# (fp32: the LDS image of those two exceeds the kernels' budget and the launch falls through to the gather-GEMM / from halop to
# halo -- the label check says so; the fp32 instantiations are reached by a thin stride-1 3x3 layer with conv3x3.hip switched off,
# a 1x1 layer, and ConvTranspose2d(4, 2, 1) 32 -> 16 at 8 x 8 (halop) / 64 -> 16 at 16 x 16 (halo))
for _name, _lab, _off in (("halop", HALP, 0), ("halo", HAL, L.K_HALOP)):
    IGEMM += _pair(_name + "/bf16", (_lab, _lab), "bf16", (3, 32, 64, 16, 3, 2, 1), halo_all=1, disable=L.K_TCONVR | L.K_SCONV | _off)
    IGEMM += [_ig(_name + "/convT/bf16", _lab, "bf16", Case("convT", 3, 64, 16, 16, 4, 2, 1, **PRO_STATS), halo_all=1, disable=L.K_TCONVR | _off)]
    IGEMM += _pair(_name + "/3x3/f32", (_lab, _lab), "f32", (4, 16, 32, 8, 3, 1, 1), halo_all=1, disable=L.K_CONV3X3 | _off)
    IGEMM += _pair(_name + "/1x1/f32", (_lab, _lab), "f32", (4, 16, 32, 8, 1, 1, 0), halo_all=1, disable=_off)
IGEMM += [_ig("halop/convT/f32", HALP, "f32", Case("convT", 3, 32, 16, 8, 4, 2, 1, **PRO_STATS), halo_all=1),
          _ig("halo/convT/f32", HAL, "f32", Case("convT", 3, 64, 16, 16, 4, 2, 1, **PRO_STATS), halo_all=1, disable=L.K_HALOP)]
IGEMM += _pair("halop/groups", (HALP, HALP), "bf16", (3, 32, 64, 16, 3, 2, 1), groups=3, halo_all=1, disable=L.K_TCONVR | L.K_SCONV)
IGEMM += _pair("halo/groups", (HAL, HAL), "bf16", (3, 32, 64, 16, 3, 2, 1), groups=3, halo_all=1, disable=L.K_TCONVR | L.K_SCONV | L.K_HALOP)
IGEMM += _pair("halo/thin-out", (None, HAL), "bf16", (3, 16, 160, 32, 3, 1, 1))
# the register-resident kernels: B = 1, 3, 70, one large batch (more than one item on a block), three groups
for _b, _g in ((1, 1), (3, 1), (70, 1), (3, 3)):
    _s = _b >= 70
    IGEMM += _pair("sconv/64-128/B%dG%d" % (_b, _g), (SCONV, TCONVR), "bf16", (_b, 64, 128, 16, 3, 2, 1), fwd_flags=PRO_STATS, groups=_g, small=_s)
    IGEMM += _pair("sconv/32-64/B%dG%d" % (_b, _g), (SCONV, TCONVX), "bf16", (_b, 32, 64, 32, 3, 2, 1), fwd_flags=PRO_STATS, groups=_g, small=_s)
    IGEMM += _pair("thconv/B%dG%d" % (_b, _g), (None, THCONV), "bf16", (_b, 16, 32, 32, 3, 1, 1), groups=_g, small=_s)
    IGEMM += [_ig("tconvr/convT/B%dG%d" % (_b, _g), TCONVR, "bf16", Case("convT", _b, 128, 64, 8, 4, 2, 1, groups=_g, small=_s, **PRO_STATS)),
              _ig("tconvx16/convT/B%dG%d" % (_b, _g), TCONVX, "bf16", Case("convT", _b, 64, 16, 16, 4, 2, 1, groups=_g, small=_s, **PRO_ONLY)),
              _ig("dconv/64/B%dG%d" % (_b, _g), DCONV, "bf16", Case("convT_dgrad", _b, 64, 16, 16, 4, 2, 1, groups=_g, small=_s, seed=3)),
              _ig("dconv/32/B%dG%d" % (_b, _g), DCONV, "bf16", Case("convT_dgrad", _b, 32, 16, 16, 4, 2, 1, groups=_g, small=_s, seed=3))]
IGEMM += _pair("sconv/32-64/B300", (SCONV, TCONVX), "bf16", (300, 32, 64, 32, 3, 2, 1), fwd_flags=PRO_STATS, small=True)
IGEMM += _pair("sconv/64-128/B300", (SCONV, TCONVR), "bf16", (300, 64, 128, 16, 3, 2, 1), fwd_flags=PRO_STATS, small=True)
IGEMM += _pair("thconv/B300", (None, THCONV), "bf16", (300, 16, 32, 32, 3, 1, 1), small=True)
IGEMM += [_ig("tconvr/convT/B300", TCONVR, "bf16", Case("convT", 300, 128, 64, 8, 4, 2, 1, small=True, **PRO_STATS)),
          _ig("tconvx16/convT/B300", TCONVX, "bf16", Case("convT", 300, 64, 16, 16, 4, 2, 1, small=True, **PRO_ONLY)),
          _ig("dconv/64/B300", DCONV, "bf16", Case("convT_dgrad", 300, 64, 16, 16, 4, 2, 1, small=True, seed=3)),
          _ig("tconvr/convT/bare", TCONVR, "bf16", Case("convT", 3, 128, 64, 8, 4, 2, 1, pro=False, bias=False, res=False, stats=False)),
          _ig("dconv/bias", DCONV, "bf16", Case("conv", 5, 16, 32, 32, 4, 2, 1, pro=False, bias=True, res=False, stats=False))]
# pconv.hip: the three shortcut shapes, groups with their own coefficients, many tiles per block
for _dims in ((3, 16, 32, 32, 1, 1, 0), (3, 32, 64, 32, 1, 2, 0), (3, 16, 160, 32, 1, 1, 0)):
    IGEMM += _pair("pconv/%d-%d" % _dims[1:3], (PCONV, None), "bf16", _dims, fwd_flags=PRO_ONLY)
IGEMM += _pair("pconv/groups", (PCONV, None), "bf16", (37, 16, 32, 32, 1, 1, 0), fwd_flags=PRO_ONLY, groups=3)
IGEMM += _pair("pconv/B130", (PCONV, None), "bf16", (130, 32, 64, 32, 1, 2, 0), fwd_flags=PRO_ONLY, groups=4, small=True)
IGEMM += _pair("pconv/bare", (PCONV, None), "bf16", (3, 16, 32, 32, 1, 1, 0), fwd_flags=dict(pro=False, bias=False, res=False, stats=False))
# pixgemm.hip: ConvTranspose2d(4, 2, 1) on 1 x 1, 2 x 2 and 4 x 4 maps and its data gradient (the LDS-halo kernels, in front of it in
# the dispatcher, switched off as in tests/test_pixgemm_gpu.py); the dispatcher's tile choice and the widest tiles
for _h, _cin, _n, _b, _g, _opts in ((1, 64, 32, 6, 1, {}), (2, 96, 128, 37, 3, {}), (4, 128, 192, 6, 1, {}), (2, 96, 128, 37, 1, dict(wide_min_blocks=1))):
    _nm = "pixel/%dx%d%s" % (_h, _h, "/widest" if _opts else "")
    IGEMM += [_ig(_nm + "/fwd", PIXEL, "bf16", Case("convT", _b, _cin, _n, _h, 4, 2, 1, groups=_g, **BARE_STATS), disable=HALO, **_opts),
              _ig(_nm + "/dgrad", PIXEL, "bf16", Case("convT_dgrad", _b, _cin, _n, _h, 4, 2, 1, groups=_g, seed=3), disable=HALO, **_opts)]
# ConvTranspose2d(4, 2, 1) through the gather-GEMM (fp32) and the LDS-DMA kernel (a plain data gradient: no epilogue)
IGEMM += [_ig("generic/convT/f32", GEN, "f32", Case("convT", 3, 128, 64, 8, 4, 2, 1, **PRO_STATS), disable=HALO),
          _ig("generic/convT-dgrad/f32", GEN, "f32", Case("convT_dgrad", 3, 128, 64, 8, 4, 2, 1, seed=3), disable=HALO),
          _ig("dma/convT-dgrad/plain", DMA, "bf16", Case("convT_dgrad", 3, 128, 64, 8, 4, 2, 1, ex=False, seed=3), wide_min_blocks=1, disable=HALO)]

LABELS = (GEN, DMA, C3, C3P, C3M, C3W, C3X, HAL, HALP, SCONV, PCONV, THCONV, TCONVR, TCONVX, DCONV, PIXEL)


def _wg(name, dt, use_tr, case, on=None, off=None, budget=0, source=""):
    return (name, dt, use_tr, case, on or {}, off, budget, source)


def _wc(kind, dims, **kw):
    B, Cin, N, H, k, s, p = dims
    return Case(kind, B, Cin, N, H, k, s, p, seed=5, **kw)


# sv_wgrad_ex has no launch label: shapes and switches are those of the existing test of each kernel (`source`), whose tolerance
# test shows (by its comparison against the kernel it replaces) that the switch selects the kernel.  on / off: the options with
# the kernel dispatched and switched off -- both must equal the reference.
WGRAD = []
for _dt, _tr in (("f32", 0), ("bf16", 0), ("bf16", 1)):
    _t = "%s/tr%d" % (_dt, _tr)
    for _dims in ((4, 16, 32, 8, 1, 1, 0), (3, 32, 64, 16, 3, 2, 1), (37, 144, 1024, 1, 1, 1, 0)):
        WGRAD.append(_wg("generic/%dx%d-%d/%s" % (_dims[4], _dims[4], _dims[1], _t), _dt, _tr, _wc("wgrad", _dims, pro=_dims[1] != 144),
                         dict(disable=L.K_HWGRAD | L.K_S2WGRAD), source="test_conv_wgrad (CONV_CASES), test_gemm_ragged_batch's shape"))
    for _dims in ((4, 32, 32, 32, 3, 1, 1), (2, 32, 96, 16, 3, 1, 1), (6, 128, 128, 8, 3, 1, 1)):
        WGRAD.append(_wg("wgrad3x3/%d-%d/%s" % (_dims[1], _dims[2], _t), _dt, _tr, _wc("wgrad", _dims), {}, dict(disable=L.K_WGRAD3X3),
                         source="test_conv_wgrad (CONV_CASES: the LDS-halo shapes)"))
WGRAD.append(_wg("wgrad3x3/groups", "bf16", 1, _wc("wgrad", (4, 32, 32, 32, 3, 1, 1), groups=3), {}, dict(disable=L.K_WGRAD3X3),
                 source="test_batched_groups_equal_separate_launches"))
for _dims in ((32, 128, 128, 8, 3, 1, 1), (8, 64, 96, 16, 3, 1, 1), (12, 64, 64, 32, 3, 1, 1)):
    WGRAD.append(_wg("wgrad3x3m/%d-%d-%d" % _dims[1:4], "bf16", 1, _wc("wgrad", _dims), {}, dict(disable=L.K_WGRAD3X3M),
                     source="test_conv_wgrad (WG_CASES: the 32x32x16 narrow kernel)"))
for _dims in ((16, 160, 160, 32, 3, 1, 1), (8, 96, 320, 16, 3, 1, 1), (32, 160, 160, 8, 3, 1, 1)):
    WGRAD.append(_wg("wgrad3x3w/%d-%d-%d" % _dims[1:4], "bf16", 1, _wc("wgrad", _dims), {}, dict(disable=L.K_WGRAD3X3W),
                     source="test_conv_wgrad (WG_CASES: wide layers)"))
for _dims in ((5, 160, 320, 32, 3, 2, 1), (7, 160, 320, 32, 1, 2, 0), (9, 160, 160, 8, 1, 1, 0)):
    WGRAD.append(_wg("wide-coop/%dx%d-%d" % (_dims[4], _dims[4], _dims[2]), "bf16", 1, _wc("wgrad", _dims, groups=3), dict(wide_min_blocks=1),
                     dict(wide_min_blocks=1, disable=L.K_WGRAD_WIDE), source="test_wide_cooperative_wgrad"))
for _dims in ((40, 16, 16, 32, 3, 1, 1), (8, 32, 64, 32, 3, 2, 1), (4, 32, 64, 16, 3, 2, 1)):
    WGRAD.append(_wg("hwgrad/%d-%d-%d" % (_dims[1], _dims[2], _dims[3]), "bf16", 1, _wc("wgrad", _dims, groups=3), dict(halo_all=1),
                     dict(halo_all=1, disable=L.K_HWGRAD), source="test_tap_fused_wgrad_conv"))
WGRAD.append(_wg("hwgrad/convT", "bf16", 1, Case("wgradT", 8, 64, 16, 16, 4, 2, 1, seed=6), dict(halo_all=1), dict(halo_all=1, disable=L.K_HWGRAD),
                 source="test_tap_fused_wgrad_convT"))
for _n, _pro in ((32, True), (16, False), (160, True)):
    for _b, _g, _bud in ((1, 1, 0), (3, 1, 0), (70, 1, 0), (33, 4, 0), (96, 2, 16)):
        WGRAD.append(_wg("thwgrad/N%d/B%dG%d" % (_n, _b, _g), "bf16", 1, _wc("wgrad", (_b, 16, _n, 32, 3, 1, 1), groups=_g, pro=_pro, small=_b >= 33),
                         {}, dict(disable=L.K_THWGRAD), _bud, source="test_thin_layers_wgrad"))
for _kind, _pro in (("wgrad", True), ("wgrad", False), ("wgradT", True)):
    for _b, _g, _bud in ((1, 1, 0), (3, 1, 0), (70, 1, 0), (33, 4, 0), (96, 2, 16), (600, 1, 0)):
        _dims = (_b, 16, 32, 32, 4, 2, 1) if _kind == "wgrad" else (_b, 32, 16, 16, 4, 2, 1)
        WGRAD.append(_wg("k4wgrad/%s%s/B%dG%d" % (_kind, "" if _pro else "/bare", _b, _g), "bf16", 1, _wc(_kind, _dims, groups=_g, pro=_pro, small=_b >= 33),
                         {}, dict(disable=L.K_THWGRAD), _bud, source="test_thin_4x4_stride2_wgrad"))
for _cin, _n, _h in ((32, 64, 32), (64, 128, 16)):
    for _b, _g, _bud, _pro in ((1, 1, 0, True), (3, 1, 0, False), (70, 1, 0, True), (33, 4, 0, True), (96, 2, 16, True), (512, 1, 256, True)):
        WGRAD.append(_wg("s2wgrad/%d-%d/B%dG%d" % (_cin, _n, _b, _g), "bf16", 1, _wc("wgrad", (_b, _cin, _n, _h, 3, 2, 1), groups=_g, pro=_pro, small=_b >= 33),
                         {}, dict(disable=L.K_S2WGRAD), _bud, source="test_banded_stride2_wgrad"))
for _dt, _tr in (("f32", 0), ("bf16", 1)):
    WGRAD.append(_wg("map4/96-160/G4/%s" % _dt, _dt, _tr, _wc("wgrad", (8, 96, 160, 4, 3, 1, 1), groups=4), {}, dict(disable=L.K_MAP4),
                     source="tests/test_preact_gpu.py test_map4_wgrad (MAP4_CASES)"))
    WGRAD.append(_wg("map4/64-96/%s" % _dt, _dt, _tr, _wc("wgrad", (24, 64, 96, 4, 3, 1, 1)), {}, dict(disable=L.K_MAP4),
                     source="tests/test_preact_gpu.py test_map4_wgrad (MAP4_CASES)"))

# sv_bwd3x3: 32 channels at 8 / 16 / 32-pixel maps, 64 channels at 16; one / two / three-tensor form; groups 1 and 4; a small budget
BWD = []
for _ch, _h in ((32, 8), (32, 16), (32, 32), (64, 16)):
    for _form in (0, 1, 2):
        BWD.append(("bwd/%d/%d/form%d" % (_ch, _h, _form), Case("bwd", 6, _ch, _ch, _h, groups=1, form=_form, seed=7 + _form), 0))
        BWD.append(("bwd/%d/%d/form%d/groups" % (_ch, _h, _form), Case("bwd", 10, _ch, _ch, _h, groups=4, form=_form, seed=17 + _form), 16))


def all_cases():
    """every Case of the three GPU tables, once"""
    seen = {}
    for row in IGEMM:
        seen.setdefault(row[3], row[0])
    for row in WGRAD:
        seen.setdefault(row[3], row[0])
    for row in BWD:
        seen.setdefault(row[1], row[0])
    return [(name, case) for case, name in seen.items()]
