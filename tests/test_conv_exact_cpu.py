"""The CPU half of the exact integer parity tests (tests/_exact.py, tests/test_conv_exact_gpu.py): the conditions under which the
GPU tests may demand equality are proven here for EVERY case of the GPU tables, the comparator is tested on itself, and one
sensitivity record shows what the tolerance tests on Gaussian operands cannot see and the exact comparison can."""
import pytest
import torch
import torch.nn.functional as F

from tests import _exact as E

CASES = E.all_cases()


@pytest.mark.parametrize("name,case", CASES, ids=[n for n, _ in CASES])
def test_preconditions_hold(name, case):
    """(a) - (f) of tests/_exact.py on the float64 reference alone"""
    E.preconditions(case)


def test_tables_cover_what_they_claim():
    names = [r[0] for r in E.IGEMM] + [r[0] for r in E.WGRAD] + [r[0] for r in E.BWD]
    assert len(names) == len(set(names)), [n for n in names if names.count(n) > 1]
    # every label sv_igemm_launch can record, each with a forward and (where the kernel has one) a data gradient
    by_label = {}
    for name, label, dt, case, opts in E.IGEMM:
        by_label.setdefault(label, set()).add(case.kind)
    assert set(by_label) == set(E.LABELS) and len(E.LABELS) == 16
    for label in E.LABELS:
        fwd, bwd = by_label[label] & {"conv", "convT"}, by_label[label] & {"conv_dgrad", "convT_dgrad"}
        if label == E.PCONV or label == E.SCONV:
            assert fwd and not bwd              # forward-only kernels
        elif label == E.THCONV:
            assert bwd and not fwd              # the activation-backward form only
        else:
            assert fwd and bwd, label
    assert any(dt == "f32" for _, _, dt, _, _ in E.IGEMM) and any(c.groups == 3 for _, _, _, c, _ in E.IGEMM)
    families = {r[0].split("/")[0] for r in E.WGRAD}
    assert families == {"generic", "wgrad3x3", "wgrad3x3m", "wgrad3x3w", "wide-coop", "hwgrad", "thwgrad", "k4wgrad", "s2wgrad", "map4"}
    assert {(c.Cin, c.H, c.form, c.groups) for _, c, _ in E.BWD} == {(ch, h, f, g) for ch, h in ((32, 8), (32, 16), (32, 32), (64, 16))
                                                                     for f in (0, 1, 2) for g in (1, 4)}


def test_comparator_reports_one_grid_unit_at_its_index():
    want = torch.arange(2 * 3 * 4 * 8, dtype=torch.float64).view(2, 3, 4, 8) - 90.0
    got = want.to(torch.bfloat16).float()
    E.assert_equal(got, want, "clean")
    got[1, 2, 3, 5] += 1.0                               # one unit of the integer grid, in one element
    with pytest.raises(AssertionError) as err:
        E.assert_equal(got, want, "one unit")
    text = str(err.value)
    assert "1 of 192 elements differ" in text and "(1, 2, 3, 5)" in text
    assert "[(2, 3)]" in text and "channels: 1 distinct [5]" in text


def test_comparator_takes_negative_zero_for_zero_and_not_nan():
    want = torch.zeros(4, dtype=torch.float64)
    E.assert_equal(torch.tensor([0.0, -0.0, 0.0, -0.0]), want, "signed zeros")
    with pytest.raises(AssertionError, match="1 of 4 elements differ"):
        E.assert_equal(torch.tensor([0.0, float("nan"), 0.0, 0.0]), want, "nan")


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def bq(t):
    return t.to(torch.bfloat16).float()


def _gaussian_forward(case):
    """the operands and reference of tests/test_kernels_gpu.py::test_conv_forward_fused, bf16"""
    B, Cin, N, H, k, stride, pad = case
    torch.manual_seed(1)
    x = bq(torch.randn(B, Cin, H, H))
    w = bq(torch.randn(N, Cin, k, k) / (Cin * k * k) ** 0.5)
    scale, shift = torch.rand(Cin) + 0.5, torch.randn(Cin) * 0.3
    bias = torch.randn(N) * 0.2
    a = bq(F.leaky_relu(x * scale[None, :, None, None] + shift[None, :, None, None], 0.01))
    res = bq(torch.randn(B, N, H, H))
    return a, w, F.conv2d(a, w, bias, stride, pad) + res


def _gaussian_wgrad(case):
    """... and of test_conv_wgrad"""
    B, Cin, N, H, k, stride, pad = case
    torch.manual_seed(5)
    x = bq(torch.randn(B, Cin, H, H))
    scale, shift = torch.rand(Cin) + 0.5, torch.randn(Cin) * 0.3
    a = bq(F.leaky_relu(x * scale[None, :, None, None] + shift[None, :, None, None], 0.01))
    dy = bq(torch.randn(B, N, H, H))
    return a, dy, torch.nn.grad.conv2d_weight(a, (N, Cin, k, k), dy, stride, pad)


# the thresholds the existing tolerance tests apply: DT["bf16"] of tests/test_kernels_gpu.py (test_conv_forward_fused, test_conv_wgrad,
# test_conv3x3_wide_*), and the 2e-3 of the register-resident weight-gradient tests (test_thin_layers_wgrad and its neighbours)
BF16_GATE, THIN_WGRAD_GATE = 2.5e-2, 2e-3


@pytest.mark.parametrize("case", [(2, 160, 160, 8, 3, 1, 1), (4, 640, 640, 8, 3, 1, 1)])
def test_sensitivity_one_missing_product_term(case):
    """One product term -- the last input channel at the centre tap (the k tail) -- missing at ONE output element: the Gaussian recipe
    with rel() passes it under the 2.5e-2 it applies (measured 1.5e-2 / 1.5e-3: the bf16 rounding of the output alone is 3.6e-3), the
    integer reference with assert_equal names the element."""
    B, Cin, N, H, k, stride, pad = case
    a, w, y = _gaussian_forward(case)
    wrong = y.clone()
    wrong[0, :, 0, 0] -= w[:, Cin - 1, 1, 1] * a[0, Cin - 1, 0, 0]
    e = rel(wrong, y)
    print("one term missing, Gaussian", case, "rel %.3e" % e)
    assert 0 < e < BF16_GATE
    c = E.Case("conv", B, Cin, N, H, k, stride, pad)
    b = E.build(c)
    act_x = E.act(b.x * 2 + b.pro[1].repeat_interleave(B, 0)[:, :, None, None])
    col = b.master[:, 4, :]                                        # the centre tap [N][Cin]
    ci = int(col.abs().sum(0).nonzero()[-1])                       # the last input channel a weight row uses there
    if float(act_x[0, ci, 0, 0]) == 0:
        pytest.fail("the chosen term is zero: pick another element")
    wrong = b.y.clone()
    wrong[0, :, 0, 0] -= col[:, ci] * act_x[0, ci, 0, 0]
    with pytest.raises(AssertionError) as err:
        E.assert_equal(E.nhwc(wrong), E.nhwc(b.y), "one term missing")
    assert "[(0, 0)]" in str(err.value)


@pytest.mark.parametrize("case,gate", [((600, 16, 32, 32, 3, 1, 1), THIN_WGRAD_GATE), ((16, 160, 160, 32, 3, 1, 1), BF16_GATE)])
def test_sensitivity_one_missing_band_edge_in_a_weight_gradient(case, gate):
    """The last image row of the last image missing from ONE tap of a weight gradient (a band edge): as a whole row rel() sees
    5.5e-3 / 4.1e-2, which the gates (2e-3 / 2.5e-2) would catch; one pixel of that row -- what a defect in one lane's address
    contributes -- stays under them.  Both are caught on the integer reference."""
    B, Cin, N, H, k, stride, pad = case
    a, dy, dw = _gaussian_wgrad(case)
    row = torch.einsum("nw,cw->nc", dy[-1, :, H - 1, :], a[-1, :, H - 1, :])
    pixel = torch.outer(dy[-1, :, H - 1, H - 1], a[-1, :, H - 1, H - 1])
    wrong_row, wrong_pixel = dw.clone(), dw.clone()
    wrong_row[:, :, 1, 1] -= row
    wrong_pixel[:, :, 1, 1] -= pixel
    e_row, e_pixel = rel(wrong_row, dw), rel(wrong_pixel, dw)
    print("band edge missing, Gaussian", case, "row rel %.3e, one pixel rel %.3e, gate %.1e" % (e_row, e_pixel, gate))
    assert 0 < e_pixel < gate
    c = E.Case("wgrad", B, Cin, N, H, k, stride, pad, small=B >= 70, seed=5)
    b = E.build(c)
    act_x = E.act(b.x * 2 + b.pro[1].repeat_interleave(B, 0)[:, :, None, None])
    for defect in (torch.einsum("nw,cw->nc", b.dy[-1, :, H - 1, :], act_x[-1, :, H - 1, :]),
                   torch.outer(b.dy[-1, :, H - 1, H - 1], act_x[-1, :, H - 1, H - 1])):
        assert bool((defect != 0).any())
        wrong = b.dw.clone()
        wrong[:, 4, :] -= defect
        with pytest.raises(AssertionError, match="elements differ"):
            E.assert_equal(E.DW0 + 2 * wrong, E.DW0 + 2 * b.dw, "band edge missing")
