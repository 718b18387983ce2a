"""The inference entry points without a GPU: the numpy restatement of sv_latent_draw's normal stream (written from the header comment of
include/shotvae_hip.h; tests/test_infer_gpu.py holds the kernel to it), the argument checks of sv_latent_draw / sv_image_out, the
eval-only API of VariationalAutoEncoder, and the CPU oracle against the reference's inference fixtures
(tests/golden/make_infer_goldens.py)."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import shot_vae_amd as S
from shot_vae_amd import _lib as L
from oracle import closed_form as CF
from oracle import shotvae_oracle as O
from tests import _cases as T
from tests import _preact_oracle as P
from tests.golden import make_infer_goldens as G
from tests.test_dropout_cpu import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5                       # tests/test_oracle_golden.py: fp32 CPU against fp32 CPU
SV_E_ARG, SV_E_SHAPE = -1, -2    # include/shotvae_hip.h


def philox_tag():
    """SV_LATENT_PHILOX_TAG of the header"""
    with open(os.path.join(ROOT, "include", "shotvae_hip.h")) as f:
        return int(re.search(r"#define\s+SV_LATENT_PHILOX_TAG\s+(0x[0-9A-Fa-f]+)u", f.read()).group(1), 16)


def latent_normals(key, row0, B, ldc, dtype=np.float64):
    """n(row0 + b, d) of sv_latent_draw for b < B, d < ldc, restated from the header comment in `dtype` arithmetic (float64: the
    reference; float32: the kernel's own precision).  The uniforms are exact in either."""
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    rows = (np.arange(B, dtype=np.uint64) + np.uint64(row0))[:, None]
    nj = (ldc + 3) // 4
    j = np.arange(nj, dtype=np.uint32)[None, :]
    lo, hi = (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32)
    r = philox4x32_10(lo + 0 * j, hi + 0 * j, j + 0 * lo, np.uint32(philox_tag()), np.uint32(k & 0xFFFFFFFF), np.uint32(k >> 32))
    out = np.empty((B, 4 * nj), dtype=dtype)
    for p in range(2):
        u1 = (((r[2 * p] >> np.uint32(8)).astype(np.int64) + 1).astype(dtype)) * dtype(2.0 ** -24)
        u2 = (r[2 * p + 1] >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)
        rad = np.sqrt(dtype(-2.0) * np.log(u1))
        ang = dtype(2.0 * math.pi) * u2
        out[:, 2 * p::4] = rad * np.cos(ang)
        out[:, 2 * p + 1::4] = rad * np.sin(ang)
    return out[:, :ldc]


def latent_z(key, row0, B, ldc, mu=None, ls=None, tau=1.0, dtype=np.float64):
    """z of sv_latent_draw in `dtype` arithmetic; tau is the value the C ABI's `float` carries"""
    if key is None:
        return np.zeros((B, ldc), dtype) if mu is None else mu.astype(dtype)
    n = latent_normals(key, row0, B, ldc, dtype)
    m = dtype(0) if mu is None else mu.astype(dtype)
    s = dtype(1) if ls is None else np.exp(ls.astype(dtype))
    return m + (dtype(np.float32(tau)) * s) * n


# ------------------------------------------------------------------------------------------------ the stream
def test_tagged_counter_never_collides_with_a_dropout_counter():
    """the dropout masks use counters (q_lo, q_hi, unit, 0); the latent stream's fourth word is the non-zero tag"""
    tag = philox_tag()
    assert 0 < tag < 2 ** 32
    c0 = np.arange(64, dtype=np.uint32)
    a = philox4x32_10(c0, 0, 3, 0, 1234, 5678)
    b = philox4x32_10(c0, 0, 3, tag, 1234, 5678)
    assert all(not np.any(x == y) for x, y in zip(a, b))


def test_rows_do_not_depend_on_the_call_they_are_drawn_in():
    for ldc in (128, 6):
        whole = latent_normals(77, 0, 12, ldc)
        parts = np.concatenate([latent_normals(77, 0, 5, ldc), latent_normals(77, 5, 7, ldc)])
        assert np.array_equal(whole, parts)
        assert not np.array_equal(whole, latent_normals(78, 0, 12, ldc))
    # a row index beyond 2^32 reaches the second counter word
    assert not np.array_equal(latent_normals(77, 1, 1, 8), latent_normals(77, 1 + 2 ** 32, 1, 8))


def test_stream_is_standard_normal_and_finite():
    """2^20 draws: the standard error of the mean is 2^-10 = 9.8e-4 and of the variance sqrt(2) * 2^-10 = 1.4e-3, so the bounds
    are about five standard errors.  u1 > 0 keeps every value finite, in fp32 as well."""
    for dtype in (np.float64, np.float32):
        n = latent_normals(0x1234567890ABCDEF, 0, 8192, 128, dtype)
        assert n.size == 2 ** 20 and np.isfinite(n).all()
        assert abs(float(n.mean(dtype=np.float64))) < 5e-3
        assert abs(float(n.var(dtype=np.float64)) - 1.0) < 1e-2
        assert float(np.abs(n).max()) <= math.sqrt(48 * math.log(2.0)) + 1e-5
    # the pairs of a generator call are uncorrelated
    n = latent_normals(5, 0, 8192, 128)
    for a, b in ((0, 1), (0, 2), (1, 3)):
        assert abs(float(np.mean(n[:, a::4] * n[:, b::4]))) < 1e-2


# ------------------------------------------------------------------------------------------------ argument checks
PTR = 4096          # never dereferenced: a refused call launches nothing


def _draw(**kw):
    a = dict(dtype=L.SV_BF16, mu=PTR, ls=PTR, key=PTR, tau=1.0, row0=0, mode=0, label=PTR, cls=None, B=4, ldc=128, K=10, Lpad=144,
             latent=PTR, z_out=None)
    a.update(kw)
    return L.lib().sv_latent_draw(a["dtype"], a["mu"], a["ls"], a["key"], a["tau"], a["row0"], a["mode"], a["label"], a["cls"], a["B"],
                                  a["ldc"], a["K"], a["Lpad"], a["latent"], a["z_out"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(latent=None), SV_E_ARG, b"latent"), (dict(dtype=2), SV_E_ARG, b"dtype"), (dict(B=0), SV_E_ARG, b"size"),
    (dict(ldc=0), SV_E_ARG, b"size"), (dict(K=-1), SV_E_ARG, b"size"), (dict(Lpad=137), SV_E_SHAPE, b"Lpad"),
    (dict(mode=3), SV_E_ARG, b"mode"), (dict(mode=-1), SV_E_ARG, b"mode"), (dict(label=None), SV_E_ARG, b"labels"),
    (dict(mode=1, cls=None), SV_E_ARG, b"class rows"), (dict(mode=2, cls=None, label=None), SV_E_ARG, b"class rows"),
    (dict(tau=-0.5), SV_E_ARG, b"tau"), (dict(tau=float("nan")), SV_E_ARG, b"tau"), (dict(tau=float("inf")), SV_E_ARG, b"tau"),
    (dict(row0=-1), SV_E_ARG, b"row0")])
def test_latent_draw_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _draw(**kw) == code and word in L.lib().sv_last_error()


def _image(**kw):
    a = dict(dtype=L.SV_BF16, inp=PTR, B=2, C=3, H=32, W=32, ld=16, sigmoid=1, f32=PTR, u8=PTR)
    a.update(kw)
    return L.lib().sv_image_out(a["dtype"], a["inp"], a["B"], a["C"], a["H"], a["W"], a["ld"], a["sigmoid"], a["f32"], a["u8"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(inp=None), SV_E_ARG, b"input"), (dict(f32=None, u8=None), SV_E_ARG, b"no output"), (dict(dtype=-1), SV_E_ARG, b"dtype"),
    (dict(B=0), SV_E_ARG, b"size"), (dict(C=0), SV_E_ARG, b"size"), (dict(H=-3), SV_E_ARG, b"size"), (dict(W=0), SV_E_ARG, b"size"),
    (dict(ld=2), SV_E_SHAPE, b"ld="), (dict(sigmoid=2), SV_E_ARG, b"sigmoid")])
def test_image_out_refuses_bad_arguments_before_any_launch(kw, code, word):
    assert _image(**kw) == code and word in L.lib().sv_last_error()


# ------------------------------------------------------------------------------------------------ API
def _model(dp=False, name="wideresnet-10-1"):
    return S.VariationalAutoEncoder(name, num_input_channels=3, img_size=(32, 32), data_parallel=dp, continuous_latent_dim=128,
                                    disc_latent_dim=10, small_input=True, compute_dtype="fp32")


def _calls(m):
    x, z, lab = torch.zeros(2, 3, 32, 32), torch.zeros(2, 128), torch.zeros(2, dtype=torch.int64)
    return {"encode": lambda: m.encode(x), "features": lambda: m.features(x), "predict": lambda: m.predict(x),
            "decode": lambda: m.decode(z, lab), "reconstruct": lambda: m.reconstruct(x), "generate": lambda: m.generate(lab, 1),
            "feature_extractor": lambda: m.feature_extractor(x),
            "feature_reconstructor": lambda: m.feature_reconstructor(torch.zeros(2, 138, 1, 1))}


def test_new_entry_points_are_eval_mode_only():
    m = _model().train()
    for name, fn in _calls(m).items():
        with pytest.raises(NotImplementedError, match=r"model\.eval\(\)"):
            fn()


def test_new_entry_points_refuse_cpu_tensors():
    m = _model().eval()
    for name, fn in _calls(m).items():
        with pytest.raises(L.ShotVaeHipError, match=r"\.%s:" % name):       # the error names the call that was made
            fn()


def test_other_sub_modules_still_raise():
    m = _model().eval()
    for name in ("global_avg", "continuous_inference", "disc_latent_inference", "sample"):
        with pytest.raises(RuntimeError, match="parameter container"):
            getattr(m, name)(torch.zeros(1))
    with pytest.raises(RuntimeError, match="parameter container"):
        m.continuous_inference.mean(torch.zeros(1))
    with pytest.raises(RuntimeError, match="parameter container"):
        m.feature_reconstructor.decoder(torch.zeros(1))


@pytest.mark.parametrize("dp", [False, True])
def test_state_dict_keys_unchanged_by_the_new_callables(dp):
    with open(os.path.join(T.GOLDEN, "ref_state_keys.json")) as f:
        ref = json.load(f)["wideresnet-10-1|K=10|dp=%d" % int(dp)]
    m = _model(dp)
    sd = m.state_dict()
    assert list(sd.keys()) == [k for k, _ in ref]
    assert all(list(sd[k].shape) == shape for k, shape in ref)
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in ref if O.is_param(k.replace(".module.", "."))]
    assert [n for n, _ in m.named_children()] == list(S.VariationalAutoEncoder.TOP_MODULES)


# ------------------------------------------------------------------------------------------------ oracle against the fixtures
def oracle_infer(name, st, inp):
    """the fixture's quantities from the CPU oracle (call under tests/_preact_oracle.patched())"""
    import torch.nn.functional as F
    with torch.no_grad():
        fmap = O.encoder_forward(st, name, inp["x"], training=False, update=False)
        feat = fmap.mean(dim=(2, 3))
        mu = F.linear(feat, st["continuous_inference.mean.fc.weight"], st["continuous_inference.mean.fc.bias"])
        ls = F.linear(feat, st["continuous_inference.log_sigma.fc.weight"], st["continuous_inference.log_sigma.fc.bias"])
        la = F.log_softmax(F.linear(feat, st["disc_latent_inference.fc.weight"], st["disc_latent_inference.fc.bias"]), dim=1)
        rec_hard = O.decoder_forward(st, inp["latent_hard"], training=False, update=False)
        rec_soft = O.decoder_forward(st, inp["latent_soft"], training=False, update=False)
    return dict(fmap=fmap, feat=feat, mu=mu, ls=ls, la=la, rec_hard=rec_hard, rec_soft=rec_soft)


@pytest.mark.parametrize("tag", list(G.CASES))
def test_oracle_reproduces_the_inference_fixtures(tag):
    name = G.CASES[tag]
    g = T.load(tag)
    with P.patched():
        out = oracle_infer(name, CF.make_state(name, K=G.K), G.infer_inputs())
    assert sorted(g.files) == sorted(out)
    for k, v in out.items():
        assert v.shape == g[k].shape and T.rel_err(v.numpy(), g[k]) < TOL, (tag, k)


# ------------------------------------------------------------------------------------------------ tools/generate_grid.py
def test_grid_tool_writes_binary_pnm(tmp_path):
    """the host side of tools/generate_grid.py: tiling and the PPM / PGM writer (numpy only)"""
    from tools import generate_grid as GG
    for ch, magic in ((3, b"P6"), (1, b"P5")):
        imgs = (np.arange(6 * 4 * 5 * ch) % 251).astype(np.uint8).reshape(6, 4, 5, ch)
        grid = GG.tile(imgs, 2, 3, pad=1)
        assert grid.shape == (2 * 5 + 1, 3 * 6 + 1, ch) and grid.dtype == np.uint8
        assert np.array_equal(grid[1:5, 1:6], imgs[0]) and np.array_equal(grid[6:10, 13:18], imgs[5])
        assert (grid[0] == 255).all() and (grid[:, 0] == 255).all() and (grid[5] == 255).all()
        path = tmp_path / ("g%d.pnm" % ch)
        GG.write_pnm(str(path), grid)
        raw = path.read_bytes()
        head = magic + b"\n%d %d\n255\n" % (grid.shape[1], grid.shape[0])
        assert raw.startswith(head) and raw[len(head):] == grid.tobytes()
