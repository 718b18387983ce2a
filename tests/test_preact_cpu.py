"""PreActResNet-18 / 34 encoders, host side (no GPU): the plan against the reference's own state_dict (tests/golden/
ref_state_keys_preact.json, written by tests/golden/make_preact_goldens.py), the name errors, the test-side oracle
(tests/_preact_oracle.py) against the reference's outputs, and the WideResNet plans unchanged."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd.engine import Plan
from oracle import closed_form as C
from oracle import shotvae_oracle as O
from tests import _cases as T
from tests import _preact_oracle as P

TOL = 2e-5          # tests/test_oracle_golden.py's tolerance for the existing oracle
SIZES = {"preactresnet18": (11168000, 121), "preactresnet34": (21276160, 217)}


def _ref_keys():
    with open(os.path.join(T.GOLDEN, "ref_state_keys_preact.json")) as f:
        return json.load(f)


def _model(name, dp):
    return S.VariationalAutoEncoder(name, num_input_channels=3, drop_rate=0, img_size=(32, 32), data_parallel=dp,
                                    continuous_latent_dim=128, disc_latent_dim=10, small_input=True)


@pytest.mark.parametrize("name", list(SIZES))
@pytest.mark.parametrize("dp", [False, True])
def test_state_dict_is_the_references(name, dp):
    ref = _ref_keys()["%s|K=10|dp=%d" % (name, int(dp))]
    sd = _model(name, dp).state_dict()
    assert list(sd.keys()) == [k for k, _ in ref]
    for k, shape in ref:
        assert list(sd[k].shape) == shape, k
    enc = [(k, s) for k, s in ref if k.startswith("feature_extractor.")]
    n_param = sum(int(np.prod(s)) for k, s in enc if O.is_param(k))
    assert (n_param, len(enc)) == SIZES[name]
    own = sum(v.numel() for k, v in sd.items() if k.startswith("feature_extractor.") and O.is_param(k))
    assert own == SIZES[name][0]


@pytest.mark.parametrize("name", list(SIZES))
def test_plan_geometry_and_slopes(name):
    p = Plan(name, K=10)
    assert p.stem_n == 64 and p.widths == [64, 128, 256, 512] and p.cfeat == 512 and p.hfeat == 4
    units = P.STAGE_UNITS[name]
    assert len(p.units) == sum(units)
    first = set(np.cumsum((0,) + units[:-1]).tolist()[1:])          # index of unit1 of stages 2, 3, 4
    for i, un in enumerate(p.units):
        assert ("convi" in un) == (i in first), i
        assert un["stride"] == (2 if i in first else 1)
        assert un["bn1"].slope == 0.0 and un["bn2"].slope == 0.0
        if "bni" in un:
            assert un["bni"].slope == 1.0          # BatchNorm without an activation (preactresnet.py:54-59)
            assert ".block%d.preact_block.unit1.i_block.norm" % (sorted(first).index(i) + 2) in un["bni"].key
    assert p.bn_t.slope == 0.0
    assert [un["hin"] for un in p.units if "convi" in un] == [32, 16, 8]
    assert all(b.slope == 0.0 for b in p.dec_bns)
    # the oracle's key table is the plan's
    with P.patched():
        sh = O.state_shapes(name)
    assert list(sh.keys()) == [k for k, _, _ in p.state_items()]


def test_name_handling():
    for n in ("preactresnet50", "preactresnet101", "preactresnet152"):
        with pytest.raises(NotImplementedError, match="bottleneck"):
            _model(n, False)
        with pytest.raises(NotImplementedError):
            Plan(n)
    for n in ("preactresnet20", "preactresnet"):
        with pytest.raises(KeyError):
            _model(n, False)
        with pytest.raises(KeyError):
            Plan(n)
    for n in ("densenet121", "resnet18", "vgg"):
        with pytest.raises(NotImplementedError):
            _model(n, False)
    with pytest.raises(ValueError):
        _model("wideresnet-28", False)
    with pytest.raises(AssertionError):
        _model("wideresnet-11-2", False)
    m = _model("wideresnet-10-1", True)
    assert "feature_extractor.encoder.wideblock1.module.wide_block.wideunit1.f_block.norm1.weight" in m.state_dict()
    assert _model("preactresnet18", False).feature_extractor.num_feature_channel == 512


def test_load_state_dict_accepts_both_layouts():
    with P.patched():
        st = C.make_state("preactresnet18")
    a, b = _model("preactresnet18", False), _model("preactresnet18", True)
    a.load_state_dict(st)
    b.load_state_dict(a.state_dict())           # plain keys into the .module. layout
    k = "feature_extractor.encoder.block4.preact_block.unit1.i_block.conv.weight"
    assert torch.equal(a.state_dict()[k], st[k])
    assert torch.equal(b.state_dict()[k.replace("block4.", "block4.module.")], st[k])
    assert torch.equal(a.flat_parameters()[0], b.flat_parameters()[0])


# (key, kind, offset, shape) of Plan.state_items() + the buffer sizes and slopes, hashed AT THE PARENT COMMIT of the change that
# made the stage list a property of the encoder family: the WideResNet plans must not move
WRN_DIGESTS = {("wideresnet-28-2", 10): "b557221afb3f3cced3af99b69b0882e5784dc2b0e259ca4279e2343e5f8afdae",
               ("wideresnet-28-10", 100): "486408d3e32abe46018ee084271b5e92e8a4cf4f24513ad97535a76a4a57ad99",
               ("wideresnet-10-1", 10): "517294a3bacbdfd92e3aff33dc75491aa74b1b133b39482dfcbfd45a99896236"}


def _plan_digest(name, K):
    p = Plan(name, K=K)
    h = hashlib.sha256()
    for key, kind, payload in p.state_items():
        if kind == "conv":
            off, shape = payload.master_off, (payload.N, payload.T, payload.Cin, payload.n_real, payload.cin_real)
        elif kind == "mat":
            off, shape = payload[0], tuple(payload[1])
        elif kind == "vec":
            off, shape = payload[0], (payload[1],)
        else:
            off, shape = {"rm": payload.rm_off, "rv": payload.rv_off, "nbt": payload.index}[kind], (payload.C,)
        h.update(repr((key, kind, off, shape)).encode())
    h.update(repr((p.n_param, p.n_buf, p.n_bnbuf, p.n_pack, [b.slope for b in p.bns])).encode())
    return h.hexdigest()


@pytest.mark.parametrize("name,K", list(WRN_DIGESTS))
def test_wideresnet_plan_unchanged(name, K):
    assert _plan_digest(name, K) == WRN_DIGESTS[(name, K)]


# ---- the test-side oracle against the reference's outputs ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SIZES))
def test_oracle_eval_forward_matches_reference(name):
    g = T.load("ref_eval_" + name.replace("resnet", ""))
    il, ll, iu, lu = C.make_batch(4, 4, 10)
    nz = C.make_noise(4, 4, 10)
    with P.patched(), torch.no_grad():
        st = C.make_state(name, K=10)
        feat = O.encoder_forward(st, name, iu, training=False)
        rec, mu, ls, la = O.vae_forward(st, name, iu, nz["eps3"], u=nz["u3"], training=False)
    assert tuple(feat.shape) == (4, 512, 4, 4)
    for k, v in (("rec", rec), ("mu", mu), ("ls", ls), ("la", la)):
        assert T.rel_err(v.numpy(), g[k]) < TOL, k


PREACT_STEP, oracle_step = P.PREACT_STEP, P.oracle_step


def test_oracle_step_matches_reference():
    """One full SHOT-VAE step of the reference (four forwards, two backwards, SGD) on preactresnet18, as tests/test_oracle_golden.py
    holds the WideResNet oracle: losses, logits, reconstructions and the mixed images at 2e-5 in fp32.

    Gradients: the reference ran in fp32, so its own rounding is the only error an EXACT restatement can show -- the oracle is run in
    fp64 and its gradient sample, parameters after SGD and BatchNorm buffers are held to the same 2e-5 (measured: 1.2e-6).  The fp32
    oracle's gradient sample is NOT a pin: its hand-written batch-statistics BatchNorm rounds differently from F.batch_norm, and with
    ReLU (gradient 0 on one side of the kink, where LeakyReLU keeps 1 %) on 8-image 4x4 maps one activation on the other side of 0
    moves single gradient entries by 1e-3 of the tensor's scale (measured: fp32 oracle against its own fp64 run 1.02e-3, against the
    reference 1.02e-3).  It is held at 2e-3, the bound test_oracle_golden.py uses for the 16 / 24-image fixtures for the same reason,
    and its per-parameter gradient norms at that file's 1e-3."""
    g = T.load("ref_step_preact18_br")
    out, st, pk = oracle_step(*PREACT_STEP)
    assert [str(n) for n in g["meta.param_names"]] == pk
    for k in T.SCALARS:
        ref = float(g["s0." + k])
        assert abs(float(out[k]) - ref) <= TOL * max(1.0, abs(ref)), (k, float(out[k]), ref)
    for k in T.TENSORS:
        assert T.rel_err(out[k].numpy(), g["s0." + k]) < TOL, k
    gr = g["s0.grad_norm"]
    assert np.all(np.abs(out["grad_norm"] - gr) <= 1e-3 * gr + 1e-6 * gr.max())
    e32 = T.rel_err(out["grad_sample"], g["s0.grad_sample"])
    print("fp32 oracle gradient sample against the reference: %.3e" % e32)
    assert e32 < 2e-3
    out, st, pk = oracle_step(*PREACT_STEP, dt=torch.float64)
    e64 = T.rel_err(out["grad_sample"], g["s0.grad_sample"])
    print("fp64 oracle gradient sample against the reference: %.3e" % e64)
    assert e64 < TOL
    assert np.all(np.abs(out["grad_norm"] - gr) <= TOL * gr + 1e-6 * gr.max())
    pn = np.array([float(st[k].detach().double().norm()) for k in pk])
    assert np.max(np.abs(pn - g["final.param_norm"]) / g["final.param_norm"]) < 1e-5
    ps = np.concatenate([st[k].detach().reshape(-1)[torch.from_numpy(T.sample_idx(st[k].numel()))].numpy() for k in pk])
    assert T.rel_err(ps, g["final.param_sample"]) < 1e-5
    for k in g.files:
        if k.startswith("final.buf."):
            assert T.rel_err(st[k[len("final.buf."):]].numpy(), g[k]) < 1e-5, k
