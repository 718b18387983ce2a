"""Host logic: the gather-GEMM geometry + weight packing reproduce torch's convolutions and their
gradients (CPU; kernels are emulated by tests/_emu.py)."""
import pytest
import torch
import torch.nn.functional as F

from shot_vae_amd import geometry as G
from tests import _emu as E


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# k, stride, pad, H, W: rectangular and odd-sized maps next to the model's square power-of-two ones
# (tests/test_conv_geometry_gpu.py runs the kernels on the same maps)
RECT_MAPS = [(3, 1, 1, 8, 16), (3, 1, 1, 16, 8), (3, 1, 1, 12, 12), (3, 1, 1, 7, 7), (3, 1, 1, 6, 10), (3, 2, 1, 12, 20),
             (3, 2, 1, 6, 20), (1, 2, 0, 6, 10), (3, 1, 1, 1, 9), (3, 1, 1, 28, 12), (4, 2, 1, 6, 10)]


@pytest.mark.parametrize("k,stride,pad,H", [(3, 1, 1, 8), (3, 2, 1, 8), (1, 1, 0, 4), (1, 2, 0, 8), (3, 1, 1, 2)])
def test_conv_forward_dgrad_wgrad(k, stride, pad, H):
    conv_forward_dgrad_wgrad(k, stride, pad, H, H)


@pytest.mark.parametrize("k,stride,pad,H,W", RECT_MAPS)
def test_conv_forward_dgrad_wgrad_rect(k, stride, pad, H, W):
    conv_forward_dgrad_wgrad(k, stride, pad, H, W)


def conv_forward_dgrad_wgrad(k, stride, pad, H, W):
    torch.manual_seed(0)
    B, Cin, N = 2, 16, 32
    x = torch.randn(B, Cin, H, W, requires_grad=True)
    w = torch.randn(N, Cin, k, k, requires_grad=True)
    y = F.conv2d(x, w, None, stride, pad)
    dy = torch.randn_like(y)
    y.backward(dy)
    master = w.detach().permute(0, 2, 3, 1).reshape(N, k * k, Cin)          # [N][T][Cin]
    gf = G.conv_like(B, H, W, Cin, N, k, stride, pad)
    out = E.emu_igemm(gf, nhwc(x.detach()), E.emu_repack(master, gf, False))
    assert out.shape[1:3] == y.shape[2:4]
    assert torch.allclose(nchw(out), y.detach(), atol=1e-4)
    gd = G.convT_like(B, H // stride, W // stride, N, Cin, k, stride, pad)   # dgrad: roles swapped
    dx = E.emu_igemm(gd, nhwc(dy), E.emu_repack(master, gd, True))
    assert dx.shape[1] == H and dx.shape[2] == W
    assert torch.allclose(nchw(dx), x.grad, atol=1e-4)
    dw = E.emu_wgrad(gf, nhwc(x.detach()), nhwc(dy))
    assert torch.allclose(dw.view(N, k, k, Cin).permute(0, 3, 1, 2), w.grad, atol=1e-3)
    if (H, W) == (1, 9):     # a one-row map: the taps of the rows above and below never land inside the image
        assert gf.phase[0].ntap == 3 and gd.phase[0].ntap == 3
    if (k, stride) == (1, 2):   # three of the four output parities of the data gradient have no tap
        assert sorted(gd.phase[i].ntap for i in range(4)) == [0, 0, 0, 1]


@pytest.mark.parametrize("H", [1, 2, 4])
def test_convT_4x4_s2_forward_dgrad_wgrad(H):
    convT_4x4_s2_forward_dgrad_wgrad(H, H)


@pytest.mark.parametrize("H,W", [(3, 5), (1, 4), (6, 2)])
def test_convT_4x4_s2_forward_dgrad_wgrad_rect(H, W):
    convT_4x4_s2_forward_dgrad_wgrad(H, W)


def convT_4x4_s2_forward_dgrad_wgrad(H, W):
    torch.manual_seed(1)
    B, Cin, N = 2, 32, 16
    x = torch.randn(B, Cin, H, W, requires_grad=True)
    w = torch.randn(Cin, N, 4, 4, requires_grad=True)                        # torch ConvT layout
    y = F.conv_transpose2d(x, w, None, 2, 1)
    dy = torch.randn_like(y)
    y.backward(dy)
    master = w.detach().permute(1, 2, 3, 0).reshape(N, 16, Cin)             # [cout][ky*4+kx][cin]
    gf = G.convT_like(B, H, W, Cin, N, 4, 2, 1)
    out = E.emu_igemm(gf, nhwc(x.detach()), E.emu_repack(master, gf, False))
    assert torch.allclose(nchw(out), y.detach(), atol=1e-4)
    gd = G.conv_like(B, 2 * H, 2 * W, N, Cin, 4, 2, 1)
    dx = E.emu_igemm(gd, nhwc(dy), E.emu_repack(master, gd, True))
    assert torch.allclose(nchw(dx), x.grad, atol=1e-4)
    dw = E.emu_wgrad(gf, nhwc(x.detach()), nhwc(dy))
    assert torch.allclose(dw.view(N, 4, 4, Cin).permute(3, 0, 1, 2), w.grad, atol=1e-3)
    if (H, W) == (1, 1):   # 1x1 input: only one of the four taps per phase can ever be inside the image
        assert all(gf.phase[p].ntap == 1 for p in range(4))


def pad_channels(t, ld):
    """[..., C] -> [..., ld] with NaN in the columns [C, ld)"""
    o = torch.full(t.shape[:-1] + (ld,), float("nan"))
    o[..., :t.shape[-1]] = t
    return o


@pytest.mark.parametrize("kind,k,stride,pad,H,W", [("conv", 3, 1, 1, 6, 10), ("conv", 3, 2, 1, 8, 8), ("convT", 4, 2, 1, 3, 5)])
def test_padded_leading_dimensions(kind, k, stride, pad, H, W):
    """ldx > Cin and ldo > N (sv_geom): the geometry carries both, columns [Cin, ldx) of the input (NaN here) do not reach the
    result, columns [N, ldo) of the output are not the layer's (the emulation leaves them zero), and the weight gradient reads
    dy with the output's leading dimension."""
    torch.manual_seed(3)
    B, Cin, N, ldx, ldo = 2, 16, 32, 16 + 8, 32 + 24
    x = torch.randn(B, Cin, H, W)
    if kind == "conv":
        w = torch.randn(N, Cin, k, k, requires_grad=True)
        y = F.conv2d(x, w, None, stride, pad)
        master = w.detach().permute(0, 2, 3, 1).reshape(N, k * k, Cin)
        g = G.conv_like(B, H, W, Cin, N, k, stride, pad, ldx=ldx, ldo=ldo)
    else:
        w = torch.randn(Cin, N, 4, 4, requires_grad=True)
        y = F.conv_transpose2d(x, w, None, 2, 1)
        master = w.detach().permute(1, 2, 3, 0).reshape(N, 16, Cin)
        g = G.convT_like(B, H, W, Cin, N, 4, 2, 1, ldx=ldx, ldo=ldo)
    assert (g.ldx, g.ldo, g.Cin, g.N) == (ldx, ldo, Cin, N)
    assert G.packed_size(g) == sum(g.phase[p].ntap for p in range(g.nphase)) * Cin * N       # (the pack does not depend on ld)
    dy = torch.randn_like(y)
    y.backward(dy)
    out = E.emu_igemm(g, pad_channels(nhwc(x), ldx), E.emu_repack(master, g, False))
    assert out.shape == (B, y.shape[2], y.shape[3], ldo)
    assert torch.allclose(nchw(out[..., :N]), y.detach(), atol=1e-4)
    assert float(out[..., N:].abs().max()) == 0.0
    dw = E.emu_wgrad(g, pad_channels(nhwc(x), ldx), pad_channels(nhwc(dy), ldo))
    ref = w.grad.permute(0, 2, 3, 1) if kind == "conv" else w.grad.permute(1, 2, 3, 0)
    assert torch.allclose(dw.view(ref.shape), ref, atol=1e-3)


def test_prologue_residual_and_padding_semantics():
    """zero padding applies AFTER BN+LeakyReLU (wideresnet.py:27-30 order)."""
    torch.manual_seed(2)
    B, C, H = 2, 16, 4
    x = torch.randn(B, C, H, H)
    w = torch.randn(C, C, 3, 3)
    scale, shift = torch.rand(C) + 0.5, torch.randn(C)
    a = F.leaky_relu(x * scale[None, :, None, None] + shift[None, :, None, None], 0.01)
    r = torch.randn(B, C, H, H)
    y = F.conv2d(a, w, None, 1, 1) + r
    g = G.conv_like(B, H, H, C, C, 3, 1, 1)
    master = w.permute(0, 2, 3, 1).reshape(C, 9, C)
    out = E.emu_igemm(g, nhwc(x), E.emu_repack(master, g, False), pro=(scale, shift, 0.01), residual=nhwc(r))
    assert torch.allclose(nchw(out), y, atol=1e-4)
