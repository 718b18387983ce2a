"""The classifier-only WideResNet baseline on a real MI355X.

Kernel level: sv_fc_fwd / sv_fc_bwd and sv_ce_fwd / sv_ce_bwd through the C ABI against float64 torch on the CPU, with the helpers and
the tolerance rule of tests/test_head_loss_kernels_gpu.py: the same formula restated in fp32 torch on the CPU, its error against
float64 measured on the test's own inputs, the kernel gets 8 x that error (floor: half an fp32 ulp).  Outputs a kernel writes start
as NaN, outputs it accumulates into start non-zero, every buffer carries a guard tail.

Model level: WideResNetClassifier / CrossEntropyLoss / classifier_train_step / GraphedClassifierStep / ClassifierEvaluator against the
reference's own outputs (tests/golden/ref_cls_*.npz, written by tests/golden/make_classifier_goldens.py) and the test-side oracle
(tests/_classifier_oracle.py) at the gates of tests/test_preact_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                     # noqa: E402
from shot_vae_amd import _lib as L           # noqa: E402
from shot_vae_amd.engine import Plan         # noqa: E402
from oracle import shotvae_oracle as O       # noqa: E402
from tests import _cases as T                # noqa: E402
from tests import _classifier_oracle as Q    # noqa: E402
from tests.test_head_loss_kernels_gpu import buf, close, dev, filled, gen, p, st, tail_untouched      # noqa: E402

FP32_TOL = 1e-3          # the project's gate for an fp32 step against the reference (tests/test_preact_gpu.py)


# ------------------------------------------------------------------------------------------------ 1. sv_fc_fwd / sv_fc_bwd
# B: one sample (a quarter of a 4-sample block) | a partial second block | two 128-sample weight-gradient slices and a remainder
# C: below the 256-channel slice of the data gradient | half of it | 2.5 slices.   K: below a wave | above it
FC_SHAPES = [(B, Cc, K) for B in (1, 5, 130) for Cc in (64, 128, 640) for K in (10, 100)]


def _fc_math(feat, W, bias, dlog, old):
    return dict(logits=F.linear(feat, W, bias), dfeat=dlog @ W, dW=old[0].to(feat.dtype) + dlog.t() @ feat,
                dbias=old[1].to(feat.dtype) + dlog.sum(0))


@functools.lru_cache(maxsize=None)
def _fc_case(B, Cc, K):
    g = gen(4000 + 7 * B + Cc + K)
    I = dict(feat=torch.randn(B, Cc, generator=g), W=torch.randn(K, Cc, generator=g) / Cc ** 0.5, bias=0.1 * torch.randn(K, generator=g),
             dlog=torch.randn(B, K, generator=g), old=(torch.randn(K, Cc, generator=g), torch.randn(K, generator=g)))
    r64 = _fc_math(I["feat"].double(), I["W"].double(), I["bias"].double(), I["dlog"].double(), I["old"])
    r32 = _fc_math(I["feat"], I["W"], I["bias"], I["dlog"], I["old"])
    return I, r64, r32


def _fc_run(I, B, Cc, K):
    d = dev()
    feat, W, bias, dlog = (I[k].to(d) for k in ("feat", "W", "bias", "dlog"))
    out = dict(logits=buf(B, K), dfeat=buf(B, Cc), dW=filled(I["old"][0]), dbias=filled(I["old"][1]))      # dfeat: NaN (written)
    L.call("sv_fc_fwd", p(feat), B, Cc, p(W), p(bias), K, p(out["logits"]), st())
    L.call("sv_fc_bwd", p(feat), B, Cc, p(W), K, p(dlog), p(out["dfeat"]), p(out["dW"]), p(out["dbias"]), st())
    torch.cuda.synchronize()
    return out


def _fc_check(out, r64, r32, B, Cc, K, tag):
    for k, n in dict(logits=B, dfeat=B, dW=K, dbias=K).items():
        close(out[k][:n], r32[k], r64[k], "fc %s %s" % (k, tag))
        tail_untouched(out[k], n, "fc %s %s" % (k, tag))


@pytest.mark.parametrize("B,Cc,K", FC_SHAPES)
def test_fc_fwd_bwd_against_float64(B, Cc, K):
    I, r64, r32 = _fc_case(B, Cc, K)
    _fc_check(_fc_run(I, B, Cc, K), r64, r32, B, Cc, K, "B=%d C=%d K=%d" % (B, Cc, K))


def test_fc_bwd_deterministic_mode():
    """the 128-sample weight-gradient slices launched one after the other: the same tolerance, and two runs bit-equal"""
    B, Cc, K = 130, 640, 100
    I, r64, r32 = _fc_case(B, Cc, K)
    with L.options(deterministic=1):
        a = _fc_run(I, B, Cc, K)
        b = _fc_run(I, B, Cc, K)
    assert not L.deterministic()
    _fc_check(a, r64, r32, B, Cc, K, "det")
    for k, n in (("logits", B), ("dfeat", B), ("dW", K), ("dbias", K)):
        assert torch.equal(a[k][:n], b[k][:n]), k + ": deterministic mode is not reproducible"


# ------------------------------------------------------------------------------------------------ 2. sv_ce_fwd / sv_ce_bwd
CE_CASES = [(B, K, False) for B in (1, 5, 130) for K in (10, 100)] + [(5, 100, True)]          # True: rows holding +-90
GOUT = 0.7          # the upstream gradient of the loss: not 1


def _ce_math(z, y, gout):
    z = z.clone().requires_grad_(True)
    row = torch.logsumexp(z, 1) - z.gather(1, y.view(-1, 1)).squeeze(1)
    loss = row.mean()
    dz, = torch.autograd.grad(loss * gout, z)
    return dict(row=row.detach(), loss=loss.detach().reshape(1), dz=dz)


def _ce_inputs(B, K, big=False):
    g = gen(5000 + 3 * B + K + int(big))
    z = 2.0 * torch.randn(B, K, generator=g)
    if big:                                   # rows that hold +90 and -90: exp overflows fp32 without the max subtraction
        z[0, 0], z[0, K - 1] = 90.0, -90.0
        z[B - 1, K // 2], z[B - 1, 1] = -90.0, 90.0
        z[B // 2] = z[B // 2] + 90.0
    y = torch.randint(0, K, (B,), generator=g)
    y[0] = 0
    y[B - 1] = K - 1                          # (B = 1: the one label is K - 1)
    return z, y


def _ce_run(z, y, B, K, with_rows=True):
    d = dev()
    zd, yd = z.to(d), y.to(d)
    gout = torch.tensor([GOUT], device=d)
    out = dict(row=buf(B), loss=buf(1), dz=buf(B, K))
    L.call("sv_ce_fwd", p(zd), p(yd), B, K, p(out["row"]) if with_rows else None, p(out["loss"]), st())
    L.call("sv_ce_bwd", p(zd), p(yd), B, K, p(gout), p(out["dz"]), st())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,K,big", CE_CASES)
def test_ce_fwd_bwd_against_float64(B, K, big):
    z, y = _ce_inputs(B, K, big)
    assert int(y.min()) == (0 if B > 1 else K - 1) and int(y.max()) == K - 1
    r64, r32 = _ce_math(z.double(), y, GOUT), _ce_math(z, y, float(np.float32(GOUT)))
    a, b = _ce_run(z, y, B, K), _ce_run(z, y, B, K, with_rows=False)
    tag = "B=%d K=%d%s" % (B, K, " +-90" if big else "")
    for k, n in dict(row=B, loss=1, dz=B).items():
        close(a[k][:n], r32[k], r64[k], "ce %s %s" % (k, tag))
        tail_untouched(a[k], n, "ce %s %s" % (k, tag))
    assert torch.isfinite(a["loss"][:1]).all()
    # the mean is one block's fixed-order sum: the same bits in two runs (default mode), with or without the row output
    assert torch.equal(a["loss"][:1], b["loss"][:1]) and torch.equal(a["dz"][:B], b["dz"][:B])
    assert torch.isnan(b["row"]).all(), "row_loss = NULL: nothing written"
    with L.options(deterministic=1):
        c = _ce_run(z, y, B, K)
    assert torch.equal(a["loss"][:1], c["loss"][:1]) and torch.equal(a["row"][:B], c["row"][:B]) and torch.equal(a["dz"][:B], c["dz"][:B])


def test_ce_label_out_of_range_is_nan_and_never_an_index():
    """a label of K in a row that is not the last and -1 in a row that is not the first (an unguarded kernel would read inside the
    tensor, and give a finite, wrong loss): those rows' losses and the mean are NaN, their gradient rows zero, every other row right"""
    B, K = 5, 10
    z, y = _ce_inputs(B, K)
    y[1], y[3] = K, -1
    good = torch.tensor([0, 2, 4])
    yc = y.clone()
    yc[1] = yc[3] = 0                          # (any valid label: rows 1 and 3 of the reference are not compared)
    r64, r32 = _ce_math(z.double(), yc, GOUT), _ce_math(z, yc, float(np.float32(GOUT)))
    out = _ce_run(z, y, B, K)
    row, dz = out["row"][:B].cpu(), out["dz"][:B].cpu()
    assert torch.isnan(row[1]) and torch.isnan(row[3]) and torch.isnan(out["loss"][0])
    assert torch.equal(dz[1], torch.zeros(K)) and torch.equal(dz[3], torch.zeros(K))
    close(row[good], r32["row"][good], r64["row"][good], "ce row, bad labels beside")
    close(dz[good], r32["dz"][good], r64["dz"][good], "ce dz, bad labels beside")
    for k, n in dict(row=B, loss=1, dz=B).items():
        tail_untouched(out[k], n, "ce %s bad labels" % k)
    # the same through the public loss: NaN, and a finite gradient
    zz = z.to(dev()).requires_grad_(True)
    loss = S.CrossEntropyLoss()(zz, y.to(dev()))
    loss.backward()
    assert torch.isnan(loss) and torch.isfinite(zz.grad).all() and torch.equal(zz.grad[1].cpu(), torch.zeros(K))


def test_cross_entropy_module():
    """S.CrossEntropyLoss(): a 0-dim tensor connected to autograd; the upstream gradient reaches sv_ce_bwd; works under no_grad"""
    B, K = 5, 10
    z, y = _ce_inputs(B, K)
    r64 = _ce_math(z.double(), y, 3.0)
    r32 = _ce_math(z, y, 3.0)
    zd = z.to(dev()).requires_grad_(True)
    crit = S.CrossEntropyLoss()
    loss = crit(zd, y.to(dev()))
    assert loss.dim() == 0 and loss.requires_grad and loss.dtype == torch.float32
    (3.0 * loss).backward()
    close(loss.detach().reshape(1), r32["loss"], r64["loss"], "CrossEntropyLoss value")
    close(zd.grad, r32["dz"], r64["dz"], "CrossEntropyLoss gradient")
    with torch.no_grad():
        l2 = crit(zd, y.to(dev()))
    assert not l2.requires_grad and torch.equal(l2, loss.detach())
    with pytest.raises(TypeError):
        crit(zd.double(), y.to(dev()))
    with pytest.raises(ValueError):
        crit(zd, y[:3].to(dev()))


# ------------------------------------------------------------------------------------------------ 3. the model
def make_model(name, K, dtype, dp=True, drop_rate=0):
    """the model with the closed-form state of the goldens, on the GPU, in training mode"""
    m = S.get_wide_resnet(name, drop_rate, input_channels=3, num_classes=K, small_input=True, data_parallel=dp, compute_dtype=dtype)
    m.load_state_dict(Q.make_state(name, K))
    return m.cuda().train()


def param_grads(model):
    return {k.replace(".module.", "."): q.grad.detach().float().cpu().clone() for k, q in model.named_parameters()}


def _batch(B, K, step=0, stream0=7000):
    image, label = Q.make_batch(B, K, step, stream0=stream0)
    return image.cuda(), label.cuda()


@pytest.mark.parametrize("tag", list(Q.STEP_CASES))
def test_steps_match_reference_golden_fp32(tag):
    """the reference's own steps (main_classifier.py:191-198 with SGD 0.1 / 0.9 / 5e-4) through classifier_train_step and FlatSGD:
    logits and loss of every step, the first step's gradients, parameters, BatchNorm buffers and counters after the last"""
    name, K, B, steps, stream0 = Q.STEP_CASES[tag]
    g = T.load(tag)
    model = make_model(name, K, "fp32", dp=True)
    crit = S.CrossEntropyLoss()
    opt = S.FlatSGD(model, **Q.SGD)
    opt.zero_grad()
    names = [str(n) for n in g["meta.param_names"]]
    for s in range(steps):
        image, label = _batch(B, K, s, stream0)
        loss, logits = S.classifier_train_step(model, crit, None if s == 0 else opt, image, label, return_outputs=True)
        torch.cuda.synchronize()
        assert logits.dtype == torch.float32 and tuple(logits.shape) == (B, K) and loss.dim() == 0
        e = T.rel_err(logits.cpu().numpy(), g["s%d.logits" % s])
        ref = float(g["s%d.loss" % s])
        print("%s step %d: logits %.3e, loss %.6f (reference %.6f)" % (tag, s, e, float(loss), ref))
        assert e < FP32_TOL, (s, e)
        assert abs(float(loss) - ref) <= FP32_TOL * max(abs(ref), 1e-6), (s, float(loss), ref)
        if s == 0:
            grads = param_grads(model)
            gn = np.array([float(grads[k].double().norm()) for k in names])
            gr = g["s0.grad_norm"]
            bad = np.abs(gn - gr) > 1e-2 * gr + 1e-4 * gr.max()
            assert not bad.any(), [(names[i], gn[i], gr[i]) for i in np.nonzero(bad)[0][:5]]
            gs = np.concatenate([grads[k].reshape(-1)[torch.from_numpy(T.sample_idx(grads[k].numel()))].numpy() for k in names])
            e_gs = T.rel_err(gs, g["s0.grad_sample"])
            print("%s grad_sample %.3e" % (tag, e_gs))
            assert e_gs < 1e-2
            S.apply_update(model, opt)          # (the step's update, after its gradients have been read)
    torch.cuda.synchronize()
    sd = {k.replace(".module.", "."): v.detach().cpu() for k, v in model.state_dict().items()}
    pn = np.array([float(sd[k].double().norm()) for k in names])
    assert np.max(np.abs(pn - g["final.param_norm"]) / g["final.param_norm"]) < 1e-3
    ps = np.concatenate([sd[k].reshape(-1)[torch.from_numpy(T.sample_idx(sd[k].numel()))].numpy() for k in names])
    assert T.rel_err(ps, g["final.param_sample"]) < 1e-3
    for k in g.files:
        if k.startswith("final.buf."):
            if k.endswith("num_batches_tracked"):
                assert int(sd[k[len("final.buf."):]]) == int(g[k]) == steps, k
            else:
                assert T.rel_err(sd[k[len("final.buf."):]].float().numpy(), g[k]) < 1e-3, k


def test_eval_matches_reference_golden():
    tag, name, K, B = Q.EVAL_CASE
    g = T.load(tag)
    model = make_model(name, K, "fp32", dp=True)
    image, label = _batch(B, K)
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "tracked" in k}
    ev = S.ClassifierEvaluator(model)
    logits, loss = ev.update(image, label)
    res = ev.result()
    assert model.training, "the evaluator restores the mode"
    assert T.rel_err(logits.cpu().numpy(), g["logits"]) < FP32_TOL
    assert abs(res["loss"] - float(g["loss"])) <= FP32_TOL * abs(float(g["loss"]))
    assert abs(res["top1"] - int(g["top1"]) / B) < 1e-6 and abs(res["top5"] - int(g["top5"]) / B) < 1e-6
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "an eval forward must not touch the running statistics"
    # two batches of different sizes: the losses are weighted by the batch sizes, the hits counted over all samples
    res2 = S.evaluate_classifier(model, [(image, label), (image[:3], label[:3])])
    with torch.no_grad():
        l3 = float(S.CrossEntropyLoss()(model.eval()(image[:3]), label[:3]))
    model.train()
    assert abs(res2["loss"] - (B * res["loss"] + 3 * l3) / (B + 3)) < 1e-5
    # a backward through an eval-mode forward raises, as the VAE's does
    out = model.eval()(image)
    with pytest.raises(NotImplementedError, match="eval-mode forward"):
        out.sum().backward()


def _oracle_step(name, K, B, dt=torch.float32, stream0=7000):
    """forward + CE + backward of the oracle (no update): logits, loss, the state with its gradients"""
    sto = Q.make_state(name, K, dt, requires_grad=True)
    image, label = Q.make_batch(B, K, 0, dt, stream0)
    logits = Q.forward(sto, name, image, training=True)
    loss = Q.cross_entropy(logits, label)
    loss.backward()
    return dict(logits=logits.detach(), loss=loss.detach()), sto


def test_step_bf16_against_reference_golden():
    """bf16 operands at the project's gates for a bf16 step: loss 5e-3, logits 3e-2 of max-abs, gradient cosine against the fp32
    oracle > 0.93 (without the stem's bias, whose true gradient is zero in front of a BatchNorm, as in the other bf16 step tests)"""
    tag = "ref_cls_step_wrn10_1"
    name, K, B, steps, stream0 = Q.STEP_CASES[tag]
    g = T.load(tag)
    model = make_model(name, K, "bf16", dp=True)
    image, label = _batch(B, K, 0, stream0)
    loss, logits = S.classifier_train_step(model, S.CrossEntropyLoss(), None, image, label, return_outputs=True)
    torch.cuda.synchronize()
    e_loss = abs(float(loss) - float(g["s0.loss"])) / abs(float(g["s0.loss"]))
    e_log = T.rel_err(logits.cpu().numpy(), g["s0.logits"])
    ref, sto = _oracle_step(name, K, B, stream0=stream0)
    grads = param_grads(model)
    pk = [k for k in sto if O.is_param(k) and not k.endswith("conv0.bias")]
    fa = torch.cat([grads[k].double().flatten() for k in pk])
    fb = torch.cat([sto[k].grad.double().flatten() for k in pk])
    cos = float(fa @ fb / fa.norm() / fb.norm())
    print("bf16 wideresnet-10-1 classifier step: loss %.3e, logits %.3e, gradient cosine %.5f" % (e_loss, e_log, cos))
    assert e_loss <= 5e-3 and e_log <= 3e-2, (e_loss, e_log)
    assert cos > 0.93, cos


def test_criterion_backward_equals_train_step():
    """loss = CrossEntropyLoss()(model(x), y); loss.backward() is the path classifier_train_step takes: the same gradients, bit for
    bit in deterministic mode"""
    name, K, B = "wideresnet-10-1", 10, 8
    image, label = _batch(B, K)
    with L.options(deterministic=1):
        a, b = make_model(name, K, "fp32"), make_model(name, K, "fp32")
        S.FlatSGD(a).zero_grad()
        S.FlatSGD(b).zero_grad()
        loss = S.CrossEntropyLoss()(a(image), label)
        loss.backward()
        loss_b = S.classifier_train_step(b, S.CrossEntropyLoss(), None, image, label)
        torch.cuda.synchronize()
    assert torch.equal(loss.detach(), loss_b)
    ga, gb = a.flat_parameters()[1], b.flat_parameters()[1]
    assert float(ga.abs().max()) > 0 and torch.equal(ga, gb)
    for (ka, pa), (kb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert ka == kb and pa.grad is not None and torch.equal(pa.grad, pb.grad), ka


def test_deterministic_mode_is_bit_identical_and_right():
    tag = "ref_cls_step_wrn10_1"
    name, K, B, steps, stream0 = Q.STEP_CASES[tag]
    g = T.load(tag)
    image, label = _batch(B, K, 0, stream0)
    flats = []
    with L.options(deterministic=1):
        for _ in range(2):
            model = make_model(name, K, "fp32")
            loss, logits = S.classifier_train_step(model, S.CrossEntropyLoss(), None, image, label, return_outputs=True)
            torch.cuda.synchronize()
            flats.append((model.flat_parameters()[1].detach().clone(), logits.clone(), loss.clone()))
            assert T.rel_err(logits.cpu().numpy(), g["s0.logits"]) < FP32_TOL
            assert abs(float(loss) - float(g["s0.loss"])) <= FP32_TOL * abs(float(g["s0.loss"]))
            grads = param_grads(model)
            names = [str(n) for n in g["meta.param_names"]]
            gn = np.array([float(grads[k].double().norm()) for k in names])
            gr = g["s0.grad_norm"]
            assert not (np.abs(gn - gr) > 1e-2 * gr + 1e-4 * gr.max()).any()
    assert all(torch.equal(x, y) for x, y in zip(*flats))


def test_graphed_step_equals_eager_step():
    """GraphedClassifierStep (forward, loss and backward captured into a hipGraph and replayed, the update eager) against the eager
    classifier_train_step with a fixed summation order, as tests/test_preact_gpu.py::test_graphed_step_equals_eager_step compares:
    after two warm-up steps and two replays every parameter and BatchNorm buffer equals the eager run's (2e-6), the counters one per
    step.  The eager step is held to the reference by the tests above."""
    name, K, B = "wideresnet-10-1", 10, 8
    state = Q.make_state(name, K)
    image, label = _batch(B, K)
    with L.options(deterministic=1):
        m1, m2 = make_model(name, K, "fp32"), make_model(name, K, "fp32")
        crit = S.CrossEntropyLoss()
        o1, o2 = S.FlatSGD(m1, lr=0.05), S.FlatSGD(m2, lr=0.05)
        o1.zero_grad()
        o2.zero_grad()
        steps, warm = 2, 2
        for _ in range(warm + steps):
            S.classifier_train_step(m1, crit, o1, image, label)
        gs = S.GraphedClassifierStep(m2, crit, o2, image, label, warmup=warm)
        for _ in range(steps):
            loss = gs()
        torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    sa, sb = m1.state_dict(), m2.state_dict()
    k0 = "encoder.wideblock3.module.wide_block.wideunit1.f_block.conv2.weight"
    moved = T.rel_err(sa[k0].cpu().numpy(), state[k0.replace(".module.", ".")].numpy())
    assert moved > 1e-4, moved
    for k in sa:
        if sa[k].dtype.is_floating_point:
            assert T.rel_err(sb[k].cpu().numpy(), sa[k].cpu().numpy()) < 2e-6, k
        else:
            assert int(sa[k]) == int(sb[k]) == warm + steps, k
    # new data through the static inputs (the returned loss is the graph's static output tensor: read it before the next replay)
    before = float(loss)
    image2, label2 = _batch(B, K, 1)
    l2 = gs(image2, label2)
    torch.cuda.synchronize()
    assert torch.isfinite(l2).all() and float(l2) != before


def test_dropout_step_matches_masked_oracle(monkeypatch):
    """drop_rate = 0.3: the step against the oracle whose norm2 inputs are multiplied by the SAME masks, regenerated from the key the
    forward recorded (sv_dropout_mask; tests/test_dropout_gpu.py's MaskedOracle, comparison and fp32 gates: loss / logits 1e-3,
    per-parameter gradients 1.5e-2 against the fp64 run, running statistics 1e-3, one BatchNorm update) -- and the eval-mode forward is
    the drop_rate = 0 model's, bit for bit."""
    from tests.test_dropout_gpu import MaskedOracle, _compare, _gate
    name, K, B = "wideresnet-10-1", 10, 8
    model = make_model(name, K, "fp32", dp=True, drop_rate=0.3)
    S.FlatSGD(model).zero_grad()
    torch.manual_seed(1234)
    image, label = _batch(B, K)
    loss, logits = S.classifier_train_step(model, S.CrossEntropyLoss(), None, image, label, return_outputs=True)
    torch.cuda.synchronize()
    keys = [int(k.item()) for k in model.last_dropout_keys]
    assert len(keys) == 1
    refs = {}
    for dt in (torch.float32, torch.float64):
        # (the oracle's encoder runs under the SHOT-VAE's key names: the masks are looked up through that plan's unit table)
        mo = MaskedOracle(monkeypatch, Plan(name, K=K), keys, p=0.3)
        refs[dt] = _oracle_step(name, K, B, dt)
        assert mo.used_all()
        monkeypatch.undo()
    out = dict(loss=loss, logits=logits)
    m = _compare(model, out, refs[torch.float32][0], refs[torch.float32][1], refs[torch.float64][1], ["loss"], ["logits"])
    print("wideresnet-10-1 classifier, dropout 0.3, fp32: cosine %.6f, worst gradient tensor %.3e (%s), loss %.3e, logits %.3e, "
          "running %.3e" % (m["cos"], m["worst"][0], m["worst"][1], m["scalar"]["loss"], m["tensor"]["logits"], m["running"]))
    _gate(m, "fp32", 1e-3, 1e-3, 1.5e-2, 1)
    # without the masks the oracle is somewhere else: the comparison above is decisive
    plain, _ = _oracle_step(name, K, B)
    assert T.rel_err(logits.cpu().numpy(), plain["logits"].numpy()) > 1e-2
    outs = []
    for p_ in (0.0, 0.3):
        me = make_model(name, K, "fp32", drop_rate=p_).eval()
        with torch.no_grad():
            outs.append(me(image).clone())
        assert me.last_dropout_keys == []
    assert torch.equal(*outs)


DP_WORKER = r'''
import os, sys, json, torch
sys.path.insert(0, %r)
import torch.distributed as dist
import shot_vae_amd as S
from shot_vae_amd import dp
from shot_vae_amd import _lib as L
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
K, B = 10, 8
L.call("sv_set_option", L.OPT_DETERMINISTIC, 1)          # fixed summation order: the comparison is down to the exchange


def make():
    torch.manual_seed(3)
    m = S.get_wide_resnet("wideresnet-10-1", 0, input_channels=3, num_classes=K, small_input=True, data_parallel=True,
                          compute_dtype="fp32").cuda().train()
    o = S.FlatSGD(m, lr=0.05, momentum=0.9, weight_decay=5e-4)
    o.zero_grad()
    return m, o


def shard_inputs(r):
    torch.manual_seed(100 + r)
    return torch.rand(B, 3, 32, 32).cuda(), torch.randint(0, K, (B,)).cuda()


crit = S.CrossEntropyLoss()
# ---- the data-parallel run: this rank's shard, one all-reduce, 1 / world in the SGD kernel, two steps ------------------------
model, opt = make()
dp.broadcast_parameters(model)
x, y = shard_inputs(rank)
for step in range(2):
    S.classifier_train_step(model, crit, opt, x, y, distributed=True)
p_dp = model._engine.param.detach().clone()
bufs_dp = model._engine.bufs.detach().clone()
if rank == 0:
    # ---- ONE process over both shards, each with its own BatchNorm statistics: the shards' backwards accumulate into the flat
    #      gradient buffer (no update in between), then one SGD step on the mean; running statistics are rank-local: rank 0's ----
    ref, ropt = make()
    for step in range(2):
        snap = ref._engine.bufs.detach().clone()
        for r in range(world):
            x_r, y_r = shard_inputs(r)
            if r > 0:
                ref._engine.bufs.copy_(snap)
            S.classifier_train_step(ref, crit, None, x_r, y_r)
            if r == 0:
                bufs0 = ref._engine.bufs.detach().clone()
        ref._engine.bufs.copy_(bufs0)
        ropt.step(grad_scale=1.0 / world)
        ropt.zero_grad()
    p_ref = ref._engine.param.detach()
    d = (p_dp - p_ref).abs().max() / p_ref.abs().max()
    db = (bufs_dp - ref._engine.bufs).abs().max() / ref._engine.bufs.abs().max()
    moved = (p_dp - make()[0]._engine.param).abs().max()
    print(json.dumps({"rel_param_diff": float(d), "rel_buf_diff": float(db), "moved": float(moved)}))
dist.barrier()
dist.destroy_process_group()
'''


@pytest.mark.timeout(900)
def test_two_rank_gloo_step_equals_single_process_over_both_shards(tmp_path):
    """Two ranks on one GPU over gloo (one all-reduce of the flat gradient buffer, 1 / world in the SGD kernel), two steps, against
    ONE process that runs both shards with their own BatchNorm statistics and steps on the mean, at the gates of the existing two-rank
    tests (1e-5).  Fresh child processes with a time limit (tests/test_dropout_gpu.py's runner)."""
    from tests.test_dropout_gpu import ROOT, _run_two_ranks
    script = tmp_path / "equiv_classifier.py"
    script.write_text(DP_WORKER % ROOT)
    res = _run_two_ranks(script, port0=31150, world=2)
    print("two ranks, wideresnet-10-1 classifier:", res)
    assert res["moved"] > 1e-4, res
    assert res["rel_param_diff"] < 1e-5, res
    assert res["rel_buf_diff"] < 1e-5, res
