"""The classifier-only WideResNet baseline, host side (no GPU): the model's state_dict against the reference's own (tests/golden/
ref_cls_state_keys.json, written by tests/golden/make_classifier_goldens.py), both key layouts, the constructor errors, the explicit
initialisation, the classifier plan, the test-side oracle (tests/_classifier_oracle.py) against the reference's outputs, and the
four new C-ABI entry points' argument checks."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from shot_vae_amd.engine import Plan
from oracle import shotvae_oracle as O
from tests import _cases as T
from tests import _classifier_oracle as Q

TOL = 2e-5          # tests/test_preact_cpu.py's tolerance for the oracle against the reference


def _ref_keys():
    with open(os.path.join(T.GOLDEN, "ref_cls_state_keys.json")) as f:
        return json.load(f)


def _model(name, K, dp, **kw):
    return S.get_wide_resnet(name, kw.pop("drop_rate", 0), input_channels=3, num_classes=K, small_input=True, data_parallel=dp, **kw)


@pytest.mark.parametrize("name,K", Q.KEY_CASES)
@pytest.mark.parametrize("dp", [False, True])
def test_state_dict_is_the_references(name, K, dp):
    ref = _ref_keys()["%s|K=%d|dp=%d" % (name, K, int(dp))]
    sd = _model(name, K, dp).state_dict()
    assert list(sd.keys()) == [k for k, _ in ref]
    for k, shape in ref:
        assert list(sd[k].shape) == shape, k


def test_wrn10_1_size():
    m = _model("wideresnet-10-1", 10, True)
    assert len(m.state_dict()) == 57
    assert sum(p.numel() for p in m.parameters()) == 77962
    assert isinstance(m, S.WideResNetClassifier)
    p, g = m.flat_parameters()
    assert p.shape == g.shape and p.dtype == torch.float32


def test_load_state_dict_accepts_both_layouts():
    st = Q.make_state("wideresnet-10-1", 10)
    a, b = _model("wideresnet-10-1", 10, False), _model("wideresnet-10-1", 10, True)
    a.load_state_dict(st)
    b.load_state_dict(a.state_dict())           # plain keys into the .module. layout
    a2 = _model("wideresnet-10-1", 10, False)
    a2.load_state_dict(b.state_dict())          # ... and back
    k = "encoder.wideblock3.wide_block.wideunit1.i_block.conv.weight"
    assert torch.equal(a.state_dict()[k], st[k])
    assert torch.equal(b.state_dict()[k.replace("wideblock3.", "wideblock3.module.")], st[k])
    assert torch.equal(b.state_dict()["classification.module.fc.weight"], st["classification.fc.weight"])
    assert torch.equal(b.state_dict()["global_avg.module.norm.running_var"], st["global_avg.norm.running_var"])
    assert torch.equal(a.flat_parameters()[0], b.flat_parameters()[0]) and torch.equal(a.flat_parameters()[0], a2.flat_parameters()[0])


def test_errors():
    for n in ("wideresnet-28", "wideresnet", "wideresnet-28-2-1"):
        with pytest.raises(ValueError):
            _model(n, 10, False)
    with pytest.raises(AssertionError, match="6n\\+4"):
        _model("wideresnet-11-2", 10, False)
    with pytest.raises(AssertionError, match="6n\\+4"):
        S.WideResNetClassifier(depth=12)
    with pytest.raises(NotImplementedError, match="small_input"):
        S.get_wide_resnet("wideresnet-10-1", 0, input_channels=3)            # the reference's default: small_input=False
    with pytest.raises(NotImplementedError, match="num_init_features"):
        S.WideResNetClassifier(depth=10, width=1, num_init_features=32)
    with pytest.raises(NotImplementedError):
        S.WideResNetClassifier(depth=10, width=1, num_input_channels=17)
    with pytest.raises(NotImplementedError, match="drop_rate == 1"):
        _model("wideresnet-10-1", 10, False, drop_rate=1)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="between 0 and 1"):
            _model("wideresnet-10-1", 10, False, drop_rate=bad)
    for kw in (dict(weight=torch.ones(10)), dict(reduction="sum"), dict(reduction="none"), dict(label_smoothing=0.1),
               dict(ignore_index=3), dict(size_average=True), dict(reduce=False)):
        with pytest.raises(NotImplementedError):
            S.CrossEntropyLoss(**kw)
    S.CrossEntropyLoss()
    m = _model("wideresnet-10-1", 10, False)
    with pytest.raises(L.ShotVaeHipError):
        m(torch.zeros(2, 3, 32, 32))                       # no CPU fallback
    with pytest.raises(L.ShotVaeHipError):
        S.CrossEntropyLoss()(torch.zeros(2, 10), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="bucket"):
        S.classifier_train_step(m, S.CrossEntropyLoss(), None, torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64),
                                distributed="bucketed")
    with pytest.raises(NotImplementedError):
        Plan("preactresnet18", head="classifier")
    with pytest.raises(ValueError):
        Plan("wideresnet-10-1", head="both")


def test_forward_signature_is_the_references():
    import inspect
    sig = inspect.signature(S.WideResNetClassifier.forward)
    assert list(sig.parameters) == ["self", "input_img", "mixup_alpha", "label", "manifold_mixup", "mixup_layer_list"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, False, None]
    sig = inspect.signature(S.get_wide_resnet)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ("drop_rate", inspect.Parameter.empty), ("input_channels", 1), ("num_classes", 10), ("small_input", False),
        ("data_parallel", True), ("compute_dtype", "bf16")]
    sig = inspect.signature(S.WideResNetClassifier.__init__)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [
        ("num_input_channels", 3), ("num_init_features", 16), ("depth", 28), ("width", 2), ("num_classes", 10), ("data_parallel", True),
        ("small_input", True), ("drop_rate", 0.0), ("compute_dtype", "bf16"), ("rng", "host")]


@pytest.mark.parametrize("name,K", [("wideresnet-10-1", 10), ("wideresnet-28-2", 100)])
def test_initialisation(name, K):
    """classifier_model/wideresnet.py:104-118: conv weights U(+-sqrt(6 / fan_in)), fc.weight U(+-sqrt(6 / (C + K))), every conv and
    fc bias 0, BatchNorm 1 / 0, running statistics 0 / 1 -- each weight inside its bound and using more than 90 % of it"""
    torch.manual_seed(5)
    sd = _model(name, K, False).state_dict()
    n_conv = 0
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 0
        elif k.endswith("running_mean"):
            assert torch.equal(v, torch.zeros_like(v))
        elif k.endswith("running_var"):
            assert torch.equal(v, torch.ones_like(v))
        elif "conv" in k and k.endswith("weight"):
            bound = math.sqrt(6.0 / (v.shape[1] * v.shape[2] * v.shape[3]))
            assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.9 * bound, k
            assert abs(float(v.mean())) < 0.2 * bound
            n_conv += 1
        elif k == "classification.fc.weight":
            bound = math.sqrt(6.0 / (v.shape[0] + v.shape[1]))
            assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.9 * bound
        elif k.endswith("bias") and ("conv" in k or "fc" in k):
            assert torch.equal(v, torch.zeros_like(v)), k
        elif "norm" in k and k.endswith("weight"):
            assert torch.equal(v, torch.ones_like(v)), k
        elif "norm" in k and k.endswith("bias"):
            assert torch.equal(v, torch.zeros_like(v)), k
        else:
            raise AssertionError("unexpected key " + k)
    assert n_conv == sum(1 for k in Q.state_shapes(name, K=K) if "conv" in k and k.endswith("weight")) >= 9
    a, b = _model(name, K, False), _model(name, K, False)          # two models draw different weights
    assert not torch.equal(a.flat_parameters()[0], b.flat_parameters()[0])


def test_classifier_plan():
    p = Plan("wideresnet-28-10", K=100, head="classifier")
    v = Plan("wideresnet-28-10", K=100)
    assert p.head == "classifier" and v.head == "vae"
    assert p.dec_convs == [] and p.dec_bns == [] and p.dec_off == p.n_param
    keys = [k for k, _, _ in p.state_items()]
    assert not any("decoder" in k or "continuous_inference" in k or "disc_latent" in k or "feature_extractor" in k for k in keys)
    assert keys[0] == "encoder.pre_process.conv0.weight" and keys[-2:] == ["classification.fc.weight", "classification.fc.bias"]
    assert p.bn_t.key == "global_avg.norm" and p.bn_t.slope == 0.01
    assert p.dp_wrapped == ("encoder.pre_process", "encoder.wideblock1", "encoder.wideblock2", "encoder.wideblock3", "global_avg",
                            "classification")
    # the same encoder: units, convolutions and BatchNorms of the VAE plan, in its order, at the same offsets
    assert len(p.units) == len(v.units) and len(p.convs) == len(v.convs) - 6 and len(p.bns) == len(v.bns) - 5
    for a, b in zip(p.convs, v.convs):
        assert (a.N, a.Cin, a.k, a.stride, a.Hin, a.master_off, a.fwd_off, a.dgrad_off) == \
               (b.N, b.Cin, b.k, b.stride, b.Hin, b.master_off, b.fwd_off, b.dgrad_off)
        assert b.key == "feature_extractor." + a.key
    assert p.n_param < v.n_param and p.n_pack < v.n_pack and p.n_buf < v.n_buf
    assert p.fc_w_off % 64 == 0 and p.fc_b_off >= p.fc_w_off + 100 * 640 and p.n_param >= p.fc_b_off + 100
    # the oracle's key table is the plan's
    assert list(Q.state_shapes("wideresnet-28-10", K=100).keys()) == keys


# ---- the test-side oracle against the reference's outputs ---------------------------------------------------------------------
def test_oracle_eval_matches_reference():
    tag, name, K, B = Q.EVAL_CASE
    g = T.load(tag)
    o = Q.run_eval(name, K, B)
    assert T.rel_err(o["logits"].numpy(), g["logits"]) < TOL
    assert abs(float(o["loss"]) - float(g["loss"])) <= TOL * max(1.0, abs(float(g["loss"])))
    assert (o["top1"], o["top5"]) == (int(g["top1"]), int(g["top5"]))
    assert 0 < int(g["top5"]) < B, "the fixture separates top-1 from top-5 and from the batch size"


@pytest.mark.parametrize("tag", list(Q.STEP_CASES))
def test_oracle_steps_match_reference(tag):
    """The reference's own steps (forward, nn.CrossEntropyLoss(), backward, SGD with momentum and weight decay): logits and loss of
    the first step at 2e-5 in fp32; everything behind a gradient -- the gradients, the logits and loss of the second step, the
    parameters after the last step and the BatchNorm buffers -- through the oracle's fp64 run at the same 2e-5, as
    tests/test_preact_cpu.py holds its oracle (the reference ran in fp32: its own rounding is the only error an exact restatement can
    show; the fp32 oracle's hand-written batch-statistics BatchNorm rounds differently from F.batch_norm, its gradient is no pin --
    measured here: the fp32 oracle's second-step logits are 1.3e-4 from the reference's, the fp64 oracle's 2.9e-7)."""
    name, K, B, steps, stream0 = Q.STEP_CASES[tag]
    g = T.load(tag)
    outs, st, pk = Q.run_steps(name, K, B, 1, stream0)
    assert [str(n) for n in g["meta.param_names"]] == pk
    assert T.rel_err(outs[0]["logits"].numpy(), g["s0.logits"]) < TOL
    assert abs(float(outs[0]["loss"]) - float(g["s0.loss"])) <= TOL * max(1.0, abs(float(g["s0.loss"])))
    outs, st, pk = Q.run_steps(name, K, B, steps, stream0, dt=torch.float64)
    for s in range(steps):
        assert T.rel_err(outs[s]["logits"].numpy(), g["s%d.logits" % s]) < TOL, s
        ref = float(g["s%d.loss" % s])
        assert abs(float(outs[s]["loss"]) - ref) <= TOL * max(1.0, abs(ref)), (s, float(outs[s]["loss"]), ref)
    gr = g["s0.grad_norm"]
    e64 = T.rel_err(outs[0]["grad_sample"], g["s0.grad_sample"])
    print("%s: fp64 oracle gradient sample against the reference: %.3e" % (tag, e64))
    assert e64 < TOL
    assert np.all(np.abs(outs[0]["grad_norm"] - gr) <= TOL * gr + 1e-6 * gr.max())
    pn = np.array([float(st[k].detach().norm()) for k in pk])
    assert np.max(np.abs(pn - g["final.param_norm"]) / g["final.param_norm"]) < TOL
    ps = np.concatenate([st[k].detach().reshape(-1)[torch.from_numpy(T.sample_idx(st[k].numel()))].numpy() for k in pk])
    assert T.rel_err(ps, g["final.param_sample"]) < TOL
    nbuf = 0
    for k in g.files:
        if k.startswith("final.buf."):
            v = st[k[len("final.buf."):]]
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(g[k]) == steps, k
            else:
                assert T.rel_err(v.numpy(), g[k]) < TOL, k
            nbuf += 1
    assert nbuf == 3 * sum(1 for k in pk if ".norm" in k and k.endswith("weight"))


def test_oracle_cross_entropy_is_torchs():
    z = torch.randn(7, 13, dtype=torch.float64)
    y = torch.arange(7) % 13
    assert abs(float(Q.cross_entropy(z, y)) - float(torch.nn.functional.cross_entropy(z, y))) < 1e-12


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
NEW = ("sv_fc_fwd", "sv_fc_bwd", "sv_ce_fwd", "sv_ce_bwd")


def test_entry_points_are_exported_and_abi_is_8():
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n) and n in L._PROTOS and n in L.EXPORTS
    assert L.lib().sv_version() == L.ABI_VERSION == 8


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """null pointers and non-positive sizes: an error code and a message, nothing launched (there is no GPU here to launch on)"""
    lib = L.lib()
    p = 4096                                   # never dereferenced
    ok = dict(sv_fc_fwd=[p, 4, 64, p, p, 10, p, None], sv_fc_bwd=[p, 4, 64, p, 10, p, p, p, p, None],
              sv_ce_fwd=[p, p, 4, 10, None, p, None], sv_ce_bwd=[p, p, 4, 10, p, p, None])
    ptrs = dict(sv_fc_fwd=(0, 3, 4, 6), sv_fc_bwd=(0, 3, 5, 6, 7, 8), sv_ce_fwd=(0, 1, 5), sv_ce_bwd=(0, 1, 4, 5))
    sizes = dict(sv_fc_fwd=(1, 2, 5), sv_fc_bwd=(1, 2, 4), sv_ce_fwd=(2, 3), sv_ce_bwd=(2, 3))
    for name in NEW:
        fn = getattr(lib, name)
        for i in ptrs[name]:
            a = list(ok[name])
            a[i] = None
            assert fn(*a) != 0 and name.encode() in lib.sv_last_error(), (name, i)
        for i in sizes[name]:
            for bad in (0, -3):
                a = list(ok[name])
                a[i] = bad
                assert fn(*a) != 0 and name.encode() in lib.sv_last_error(), (name, i, bad)
    # shapes whose rows do not fit the block's LDS are refused too
    assert lib.sv_fc_fwd(p, 4, 1 << 20, p, p, 10, p, None) != 0 and b"too large" in lib.sv_last_error()
    assert lib.sv_fc_bwd(p, 4, 64, p, 1 << 20, p, p, p, p, None) != 0 and b"too large" in lib.sv_last_error()
