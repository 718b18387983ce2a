"""The smooth-ELBO inference entry points without a GPU: the argument checks of sv_smooth_classify, the new callables of SmoothVAE /
SmoothEvaluator on CPU tensors, the unchanged state dict, the CPU oracle against the reference's inference fixtures
(tests/golden/make_smooth_eval_goldens.py) -- which pins the oracle the GPU tests' allowances are measured from -- and the host side
of tools/smooth_grid.py."""
import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from oracle import smooth_oracle as SO
from tests import _cases as T
from tests import _smooth_infer as SI
from tests.golden import make_smooth_eval_goldens as G

TOL = 2e-5                       # tests/test_oracle_golden.py: fp32 CPU against fp32 CPU
SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h
PTR = 4096                       # never dereferenced: a refused call launches nothing


def _classify(**kw):
    a = dict(dtype=L.SV_BF16, o=PTR, ldo=80, B=4, Dc=32, Dd=10, label=PTR, alpha=PTR, pred=PTR, counts=PTR, confusion=PTR)
    a.update(kw)
    return L.lib().sv_smooth_classify(a["dtype"], a["o"], a["ldo"], a["B"], a["Dc"], a["Dd"], a["label"], a["alpha"], a["pred"],
                                      a["counts"], a["confusion"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(o=None), SV_E_ARG, b"o is NULL"),
    (dict(alpha=None, pred=None, counts=None, confusion=None), SV_E_ARG, b"no output"),
    (dict(alpha=None, pred=None, counts=None, confusion=None, label=None), SV_E_ARG, b"no output"),
    (dict(label=None), SV_E_ARG, b"labels"), (dict(label=None, confusion=None), SV_E_ARG, b"labels"),
    (dict(label=None, counts=None), SV_E_ARG, b"labels"),
    (dict(B=0), SV_E_ARG, b"size"), (dict(B=-3), SV_E_ARG, b"size"), (dict(Dc=0), SV_E_ARG, b"size"), (dict(Dd=0), SV_E_ARG, b"size"),
    (dict(Dd=-1), SV_E_ARG, b"size"), (dict(ldo=73), SV_E_SHAPE, b"ldo"), (dict(ldo=0), SV_E_SHAPE, b"ldo"),
    (dict(dtype=2), SV_E_ARG, b"dtype"), (dict(dtype=-1), SV_E_ARG, b"dtype")])
def test_smooth_classify_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _classify(**kw) == code and word in L.lib().sv_last_error()


def test_smooth_classify_is_bound_and_exported():
    assert "sv_smooth_classify" in L.EXPORTS and hasattr(L.lib(), "sv_smooth_classify")
    assert L.lib().sv_version() == L.ABI_VERSION == 8
    for name in ("SmoothEvaluator", "evaluate_smooth"):
        assert hasattr(S, name)


def _model(kind="svhn", train=True):
    m = S.SmoothVAE((SO.KINDS[kind]["in_ch"], 32, 32), {"cont": 32, "disc": [10]}, compute_dtype="fp32")
    return m.train(train)


@pytest.mark.parametrize("train", [True, False])
def test_new_callables_refuse_cpu_tensors(train):
    m = _model(train=train)
    x, z, lab = torch.zeros(2, 3, 32, 32), torch.zeros(2, 32), torch.zeros(2, dtype=torch.int64)
    calls = {"classify": lambda: m.classify(x), "predict": lambda: m.predict(x), "reconstruct": lambda: m.reconstruct(x),
             "reconstruct(label)": lambda: m.reconstruct(x, lab), "generate": lambda: m.generate(lab, 1),
             "traverse": lambda: m.traverse(z, lab), "traverse(dim)": lambda: m.traverse(z, lab, dim=0, values=[0.0, 1.0]),
             "SmoothEvaluator.update": lambda: S.SmoothEvaluator(m).update(x, lab),
             "evaluate_smooth": lambda: S.evaluate_smooth(m, [(x, lab)])}
    for name, fn in calls.items():
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            fn()
    with pytest.raises(ValueError, match="label"):            # a continuous traversal needs the class it runs under
        m.traverse(z, None, dim=0, values=[0.0])
    assert m.training == train
    assert S.SmoothEvaluator(m).result()["total"] == 0


@pytest.mark.parametrize("kind", G.KINDS)
def test_state_dict_keys_unchanged_by_the_new_callables(kind):
    m = _model(kind)
    ref = SO.state_shapes(kind)
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert all(tuple(sd[k].shape) == tuple(ref[k]) for k in ref)
    assert [k for k, _ in m.named_parameters()] == list(ref.keys())


@pytest.mark.parametrize("kind", G.KINDS)
def test_oracle_reproduces_the_smooth_inference_fixtures(kind):
    """oracle.smooth_oracle.forward(training=False) on the regenerated inputs against the reference's own outputs; the restated
    forward of tests/_smooth_infer.py (what the GPU tests' allowances come from) is the same function in fp32"""
    c = SI.case(kind)
    g, o = c["g"], c["oracle"]
    assert sorted(g) == ["alpha", "hits", "label", "logits", "pred", "rec", "rec_label", "rec_latent"]
    assert g["alpha"].shape == (256, 10) and g["rec"].shape == (G.N_REC, SO.KINDS[kind]["in_ch"], 32, 32)
    for k in ("alpha", "logits", "rec", "rec_label", "rec_latent"):
        e = T.rel_err(o[k].numpy(), g[k])
        assert o[k].shape == g[k].shape and e < TOL, (kind, k, e)
    assert np.array_equal(o["pred"].numpy(), g["pred"]) and np.array_equal(g["pred"], g["alpha"].argmax(1))
    # the labels and the hit count the reference's comparison gave
    assert np.array_equal(g["label"], G.eval_labels(torch.from_numpy(g["pred"])).numpy())
    assert int(g["hits"]) == int((g["pred"] == g["label"]).sum()) == 256 - len(range(0, 256, 3))
    # the allowances of the GPU tests, measured here on the CPU: the undecided rows are a minority
    print("FIG %s gap %.4f undecided %d tol_alpha %.2e tol_rec %.2e %.2e %.2e" % (
        kind, c["gap"], int((~c["decided"]).sum()), c["tol_alpha"], c["tol_rec"], c["tol_rec_label"], c["tol_rec_latent"]))
    assert int((~c["decided"]).sum()) <= SI.MAX_UNDECIDED
    assert len(set(g["pred"][c["decided"]].tolist())) >= 5, "the decided rows cover several classes"


def test_smooth_grid_writes_binary_pnm(tmp_path):
    """the host side of tools/smooth_grid.py on a CPU-built grid: [-1, 1] -> uint8, tiling, the PPM / PGM file"""
    from tools import smooth_grid as SG
    for ch, magic in ((3, b"P6"), (1, b"P5")):
        img = torch.linspace(-1.0, 1.0, 6 * ch * 4 * 5).reshape(6, ch, 4, 5)
        u8 = SG.to_u8(img)
        assert u8.shape == (6, 4, 5, ch) and u8.dtype == np.uint8 and u8.min() == 0 and u8.max() == 255
        assert np.array_equal(u8, np.floor((img.permute(0, 2, 3, 1).numpy() + 1.0) * 127.5 + 0.5).astype(np.uint8))
        path = tmp_path / ("s%d.pnm" % ch)
        SG.save_grid(str(path), img, 2, 3)
        raw = path.read_bytes()
        w, h = 3 * (5 + 2) + 2, 2 * (4 + 2) + 2
        head = magic + b"\n%d %d\n255\n" % (w, h)
        assert raw.startswith(head) and len(raw) == len(head) + w * h * ch
        grid = np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(h, w, ch)
        assert np.array_equal(grid[2:6, 2:7], u8[0]) and np.array_equal(grid[8:12, 16:21], u8[5]) and (grid[0] == 255).all()
