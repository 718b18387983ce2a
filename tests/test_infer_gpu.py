"""The inference entry points on a real MI355X.

Kernel level: sv_latent_draw and sv_image_out through the C ABI against float64 numpy (the stream's restatement of
tests/test_infer_cpu.py, written from the header comment).  Exact quantities -- the class part, the pad columns, the logits, the
uint8 pixels, every bit-for-bit property -- are compared exactly; transcendental outputs by the house rule of
tests/test_head_loss_kernels_gpu.py: the kernel gets 8 x the error of an fp32 numpy restatement against the float64 one (at least
8 x 2^-24), max |a - ref| / max |ref| over the tensor, measured here on the test's own inputs.

Model level (fp32 mode unless said otherwise): encode / features / feature_extractor / feature_reconstructor against the reference's
fixtures (tests/golden/make_infer_goldens.py), the new calls against the existing eval model(x), generate / reconstruct against the
restated stream, state and gradients untouched, a training step afterwards equal to a fresh model's, bf16 against fp32, and
generate under graph capture."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from oracle import closed_form as CF                            # noqa: E402
from oracle import shotvae_oracle as O                          # noqa: E402
from tests import _cases as T                                   # noqa: E402
from tests import _preact_oracle as P                           # noqa: E402
from tests.golden import make_infer_goldens as G                # noqa: E402
from tests.test_infer_cpu import latent_z                       # noqa: E402
from tests.test_model_gpu import FP32_TOL, make_model           # noqa: E402

DT = {"f32": (L.SV_F32, torch.float32), "bf16": (L.SV_BF16, torch.bfloat16)}
HALF_ULP = 2.0 ** -24
GUARD = 2
NAN = float("nan")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def close(got, f32, ref, what):
    """the house rule: kernel error <= 8 x max(error of the fp32 restatement, 2^-24); prints the figures"""
    assert np.isfinite(got).all(), what + ": non-finite value (element not written)"
    cpu, e = rel(f32, ref), rel(got, ref)
    lim = 8.0 * max(cpu, HALF_ULP)
    print("FIG %-40s cpu32 %.3e kernel %.3e allow %.3e" % (what, cpu, e, lim))
    assert e <= lim, "%s: kernel error %g > 8 x the fp32 restatement's %g" % (what, e, cpu)


def dev_t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


# ================================================================================================ sv_latent_draw
def draw(dt, B, ldc, K, Lpad, mu=None, ls=None, key=None, tau=1.0, row0=0, mode=0, label=None, cls=None):
    """one sv_latent_draw call into NaN-filled buffers with guard rows -> (latent [B, Lpad] as float64 numpy, z [B, ldc] fp32 numpy)"""
    code, tt = DT[dt]
    latent = torch.full((B + GUARD, Lpad), NAN, dtype=tt, device=dev())
    z = torch.full((B + GUARD, ldc), NAN, dtype=torch.float32, device=dev())
    L.call("sv_latent_draw", code, p(mu), p(ls), p(key), float(tau), int(row0), mode, p(label), p(cls), B, ldc, K, Lpad, p(latent), p(z),
           st())
    torch.cuda.synchronize()
    assert torch.isnan(latent[B:].float()).all() and torch.isnan(z[B:]).all(), "guard rows written"
    return latent[:B].double().cpu().numpy(), z[:B].cpu().numpy()


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()


# (B, ldc, K, Lpad, row0): the model's shape | ldc no multiple of 4 | more rows than one block holds threads, K > 64, ldc % 4 == 0 but
# 100 / 4 = 25 groups | one row.  row0 of the first: the rows cross 2^32, the second counter word.
DRAW_SHAPES = [(5, 128, 10, 144, 2 ** 32 - 2), (3, 6, 10, 16, 0), (130, 100, 100, 208, 7), (1, 128, 10, 144, 3)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,ldc,K,Lpad,row0", DRAW_SHAPES)
def test_latent_draw_against_float64(dt, B, ldc, K, Lpad, row0):
    rng = np.random.default_rng(1000 + B + ldc)
    mu = (rng.standard_normal((B, ldc)) * 0.7).astype(np.float32)
    ls = (rng.standard_normal((B, ldc)) * 0.3 - 0.5).astype(np.float32)
    label = ((np.arange(B) * 7 + 3) % K).astype(np.int64)
    label[0] = K                                   # out of range: no class
    if B > 2:
        label[2] = -1
    cls = rng.random((B, K)).astype(np.float32)
    cls[0, [K - 2, 1, 4]] = 2.0                    # a three-way tie of the maximum: index 1 wins
    keyv = 0x0123456789ABCDEF
    d_mu, d_ls, d_label, d_cls = dev_t(mu), dev_t(ls), dev_t(label), dev_t(cls)
    key = torch.tensor([keyv], dtype=torch.int64, device=dev())
    onehot = np.zeros((B, K))
    for b in range(B):
        if 0 <= label[b] < K:
            onehot[b, label[b]] = 1.0
    exact = (lambda a: a) if dt == "f32" else bf16_round
    tag = "latent_draw %s B=%d ldc=%d" % (dt, B, ldc)

    # --- z against float64, the latent's z part = the fp32 z rounded once, class mode 0, the pad
    for tau in (0.0, 0.7, 1.0):
        lat, z = draw(dt, B, ldc, K, Lpad, d_mu, d_ls, key, tau, row0, 0, d_label)
        close(z, latent_z(keyv, row0, B, ldc, mu, ls, tau, np.float32), latent_z(keyv, row0, B, ldc, mu, ls, tau), "%s tau=%g z" % (tag, tau))
        assert np.array_equal(lat[:, :ldc], exact(z)), "latent z part is not the rounding of the fp32 z"
        assert np.array_equal(lat[:, ldc:ldc + K], onehot), "class part, mode 0"
        assert np.all(lat[:, ldc + K:] == 0.0), "pad columns"
        if tau == 0.0:
            assert np.array_equal(z, mu)
    # --- class modes 1 and 2 (the z part does not depend on the mode)
    lat1, z1 = draw(dt, B, ldc, K, Lpad, d_mu, d_ls, key, 1.0, row0, 1, None, d_cls)
    assert np.array_equal(z1, z) and np.array_equal(lat1[:, ldc:ldc + K], exact(cls)) and np.all(lat1[:, ldc + K:] == 0.0)
    lat2, z2 = draw(dt, B, ldc, K, Lpad, d_mu, d_ls, key, 1.0, row0, 2, None, d_cls)
    want = np.zeros((B, K))
    want[np.arange(B), np.argmax(cls, axis=1)] = 1.0         # numpy's argmax: the first = lowest index of the maximum
    assert int(np.argmax(cls[0])) == 1
    assert np.array_equal(z2, z) and np.array_equal(lat2[:, ldc:ldc + K], want) and np.all(lat2[:, ldc + K:] == 0.0)
    # --- null mu, null ls, null key
    _, zm = draw(dt, B, ldc, K, Lpad, None, d_ls, key, 0.7, row0, 0, d_label)
    close(zm, latent_z(keyv, row0, B, ldc, None, ls, 0.7, np.float32), latent_z(keyv, row0, B, ldc, None, ls, 0.7), tag + " null mu")
    _, zs = draw(dt, B, ldc, K, Lpad, d_mu, None, key, 0.7, row0, 0, d_label)
    close(zs, latent_z(keyv, row0, B, ldc, mu, None, 0.7, np.float32), latent_z(keyv, row0, B, ldc, mu, None, 0.7), tag + " null ls")
    _, zn = draw(dt, B, ldc, K, Lpad, None, None, key, 1.0, row0, 0, d_label)
    close(zn, latent_z(keyv, row0, B, ldc, dtype=np.float32), latent_z(keyv, row0, B, ldc), tag + " n")
    latk, zk = draw(dt, B, ldc, K, Lpad, d_mu, d_ls, None, 1.0, row0, 0, d_label)
    assert np.array_equal(zk, mu) and np.array_equal(latk[:, :ldc], exact(mu)), "null key: z == mu exactly"
    _, z0 = draw(dt, B, ldc, K, Lpad, None, d_ls, None, 1.0, row0, 0, d_label)
    assert np.all(z0 == 0.0)
    # --- rows drawn in several calls equal the rows drawn in one, bit for bit
    if B > 1:
        b1 = B // 2
        la_, za = draw(dt, b1, ldc, K, Lpad, d_mu[:b1], d_ls[:b1], key, 1.0, row0, 0, d_label[:b1])
        lb_, zb = draw(dt, B - b1, ldc, K, Lpad, d_mu[b1:], d_ls[b1:], key, 1.0, row0 + b1, 0, d_label[b1:])
        lat, z = draw(dt, B, ldc, K, Lpad, d_mu, d_ls, key, 1.0, row0, 0, d_label)
        assert np.array_equal(np.concatenate([za, zb]), z) and np.array_equal(np.concatenate([la_, lb_]), lat)
    # --- the key is read on the device: another key, another draw; the same key, the same bits
    lat_a, z_a = draw(dt, B, ldc, K, Lpad, d_mu, d_ls, key, 1.0, row0, 0, d_label)
    key.fill_(keyv + 1)
    lat_b, z_b = draw(dt, B, ldc, K, Lpad, d_mu, d_ls, key, 1.0, row0, 0, d_label)
    key.fill_(keyv)
    lat_c, z_c = draw(dt, B, ldc, K, Lpad, d_mu, d_ls, key, 1.0, row0, 0, d_label)
    assert not np.array_equal(z_a, z_b) and float(np.mean(z_a != z_b)) > 0.99
    close(z_b, latent_z(keyv + 1, row0, B, ldc, mu, ls, 1.0, np.float32), latent_z(keyv + 1, row0, B, ldc, mu, ls, 1.0), tag + " key + 1")
    assert np.array_equal(z_a, z_c) and np.array_equal(lat_a, lat_c)


# ================================================================================================ sv_image_out
def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B,Cc,H,W,ld", [(3, 3, 32, 32, 16), (2, 1, 32, 32, 16), (5, 3, 32, 32, 16)])
def test_image_out_against_float64(dt, B, Cc, H, W, ld):
    code, tt = DT[dt]
    rng = np.random.default_rng(50 + B + Cc)
    x = torch.from_numpy((rng.standard_normal((B, H, W, ld)) * 3.0).astype(np.float32))
    x[0, 0, :8, 0] = torch.tensor([20.0, -20.0, 90.0, -90.0, 0.0, -0.0, 104.0, -104.0])      # saturation; expf(104) overflows
    x = x.to(tt).float().numpy()                   # the values the kernel reads, exact in either dtype
    # a pixel value within 1e-3 of a rounding boundary of floor(255 s + 0.5) is replaced: exact equality is then a fair demand of an
    # fp32 sigmoid (error ~1e-7 x 255)
    v = 255.0 * sigmoid64(x)
    near = np.abs(v - np.floor(v) - 0.5) < 1e-3
    x[near] = 0.25
    v = 255.0 * sigmoid64(x)
    assert not (np.abs(v - np.floor(v) - 0.5) < 1e-3).any()
    d_x = dev_t(x, tt)
    xs = x[..., :Cc]
    want_logit = np.transpose(xs, (0, 3, 1, 2))
    want_sig = sigmoid64(want_logit)
    x32 = want_logit.astype(np.float32)
    with np.errstate(over="ignore"):                       # exp(104) = inf in fp32, as in the kernel: s = 0
        sig32 = np.float32(1.0) / (np.float32(1.0) + np.exp(-x32))
    want_u8 = np.floor(255.0 * sigmoid64(xs) + 0.5).astype(np.uint8)

    def run(sigmoid, want_f32, want_u8_):
        f32 = torch.full((B + GUARD, Cc, H, W), NAN, dtype=torch.float32, device=dev()) if want_f32 else None
        u8 = torch.full((B + GUARD, H, W, Cc), 77, dtype=torch.uint8, device=dev()) if want_u8_ else None
        L.call("sv_image_out", code, p(d_x), B, Cc, H, W, ld, sigmoid, p(f32), p(u8), st())
        torch.cuda.synchronize()
        assert f32 is None or torch.isnan(f32[B:]).all(), "guard rows written"
        assert u8 is None or bool((u8[B:] == 77).all()), "guard rows written"
        return (f32[:B].cpu().numpy() if want_f32 else None), (u8[:B].cpu().numpy() if want_u8_ else None)

    tag = "image_out %s B=%d C=%d" % (dt, B, Cc)
    logit, _ = run(0, True, False)
    assert np.array_equal(logit, want_logit), "logits are copied exactly"
    sig, _ = run(1, True, False)
    close(sig, sig32, want_sig, tag + " sigmoid")
    _, u8 = run(1, False, True)
    assert np.array_equal(u8, want_u8), "uint8 pixels: %d differ" % int((u8 != want_u8).sum())
    for flag, f_alone in ((0, logit), (1, sig)):            # both outputs in one call = each on its own
        f_both, u_both = run(flag, True, True)
        assert np.array_equal(f_both, f_alone) and np.array_equal(u_both, want_u8)


# ================================================================================================ model level
def infer_model(name, K=G.K, dtype="fp32", dp=False):
    with P.patched():
        state = CF.make_state(name, K=K)
    return make_model(name, K, dtype, state, dp).eval(), state


def terr(t, ref):
    return T.rel_err(t.detach().float().cpu().numpy(), ref.detach().float().cpu().numpy() if torch.is_tensor(ref) else ref)


@pytest.mark.parametrize("dp", [False, True])
@pytest.mark.parametrize("tag", list(G.CASES))
def test_new_calls_match_the_reference(tag, dp):
    g = T.load(tag)
    model, _ = infer_model(G.CASES[tag], dp=dp)
    inp = {k: v.cuda() for k, v in G.infer_inputs().items()}
    mu, ls, la = model.encode(inp["x"])
    got = dict(mu=mu, ls=ls, la=la, feat=model.features(inp["x"]), fmap=model.feature_extractor(inp["x"]),
               rec_hard=model.feature_reconstructor(inp["latent_hard"]), rec_soft=model.feature_reconstructor(inp["latent_soft"]))
    for k, v in got.items():
        assert tuple(v.shape) == g[k].shape and not v.requires_grad, k
        e = terr(v, g[k])
        print("FIG %s dp=%d %-9s %.3e" % (tag, dp, k, e))
        assert e < FP32_TOL, (tag, k, e)
    assert torch.equal(model.predict(inp["x"]), la.argmax(dim=1)) and model.predict(inp["x"]).dtype == torch.int64
    # decode's two class forms are feature_reconstructor's
    assert terr(model.decode(inp["z"], inp["label"]), g["rec_hard"]) < FP32_TOL
    assert terr(model.decode(inp["z"], inp["soft"]), g["rec_soft"]) < FP32_TOL


def _eval_forward(model, x, eps, **kw):
    with torch.no_grad(), T.scripted_rng(randn=[eps] * 1, rand=[] if "disc_label" in kw else [torch.rand(x.size(0), model._plan.K)]):
        return model(x, **kw)


@pytest.mark.parametrize("name", ["wideresnet-10-1", "preactresnet18"])
def test_encode_and_decode_are_the_halves_of_the_eval_forward(name):
    model, _ = infer_model(name)
    B = 6
    x = CF.uniform((B, 3, 32, 32), 7100).cuda()
    eps = CF.normal((B, 128), 7101)
    label = ((torch.arange(B) * 3 + 2) % G.K).cuda()
    with L.options(deterministic=1):
        rec, mu, ls, la = _eval_forward(model, x, eps, disc_label=label)
        emu, els, ela = model.encode(x)
        assert torch.equal(emu, mu) and torch.equal(els, ls) and torch.equal(ela, la), "deterministic mode: encode != model(x)"
    # default mode: no further off than two eval forwards are from each other (8 x, at least 1e-6)
    o1, o2 = _eval_forward(model, x, eps, disc_label=label), _eval_forward(model, x, eps, disc_label=label)
    enc = model.encode(x)
    for i, k in ((1, "mu"), (2, "ls"), (3, "la")):
        d = terr(o2[i], o1[i])
        e = terr(enc[i - 1], o1[i])
        print("FIG %s %s: model(x) twice %.3e, encode %.3e" % (name, k, d, e))
        assert e <= max(8 * d, 1e-6), (k, e, d)
    # decode from the same latent: z = mu + exp(ls) * eps formed outside
    z = mu + torch.exp(ls) * eps.cuda()
    e = terr(model.decode(z, label), rec)
    print("FIG %s decode against rec of model(x, disc_label): %.3e" % (name, e))
    assert e < FP32_TOL


def test_generate_and_reconstruct():
    model, state = infer_model("wideresnet-10-1")
    eng = model._engine
    B, keyv = 12, 987654321012345
    labels = ((torch.arange(B) * 5 + 1) % G.K).cuda()
    z64 = latent_z(keyv, 0, B, 128, tau=0.8)
    img = model.generate(labels, keyv, tau=0.8)
    assert tuple(img.shape) == (B, 3, 32, 32) and img.dtype == torch.float32 and not img.requires_grad
    want = torch.sigmoid(model.decode(dev_t(z64.astype(np.float32)), labels))
    e = terr(img, want)
    print("FIG generate against sigmoid(decode(z restated)): %.3e" % e)
    assert e < FP32_TOL
    assert terr(model.decode(dev_t(z64.astype(np.float32)), labels, sigmoid=True), want) < FP32_TOL
    # uint8: the rounding of the same images (a value within the fp32 gate of a rounding boundary may land on either side)
    u8 = model.generate(labels, keyv, tau=0.8, dtype="uint8")
    assert tuple(u8.shape) == (B, 32, 32, 3) and u8.dtype == torch.uint8
    assert float((u8.permute(0, 3, 1, 2).float() - 255.0 * img).abs().max()) <= 0.5 + 255.0 * FP32_TOL
    key = torch.tensor([keyv], dtype=torch.int64, device="cuda")
    with L.options(deterministic=1):
        a, b = model.generate(labels, key, tau=0.8), model.generate(labels, keyv, tau=0.8)
        assert torch.equal(a, b), "one key, two calls (device key and int key): not bit-identical"
        assert torch.equal(model.generate(labels, key, tau=0.8, dtype="uint8"), model.generate(labels, key, tau=0.8, dtype="uint8"))
    # 12 rows in one call against 5 + 7 with row0: z bitwise, images within the fp32 gate (the tile dispatch may differ with B)
    _, z12 = eng.latent_draw(12, key=key, tau=0.8, label=labels, want_z=True)
    _, z5 = eng.latent_draw(5, key=key, tau=0.8, label=labels[:5].contiguous(), want_z=True)
    _, z7 = eng.latent_draw(7, key=key, tau=0.8, row0=5, label=labels[5:].contiguous(), want_z=True)
    assert torch.equal(z12, torch.cat([z5, z7]))
    close(z12.cpu().numpy(), latent_z(keyv, 0, B, 128, tau=0.8, dtype=np.float32), z64, "engine latent_draw z")
    parts = torch.cat([model.generate(labels[:5], key, tau=0.8), model.generate(labels[5:], key, tau=0.8, row0=5)])
    e = terr(parts, img)
    print("FIG generate 5 + 7 rows against 12: %.3e" % e)
    assert e < FP32_TOL
    # reconstruct: the posterior mean under another class = decode(mu, other); under the predicted class by default
    x = CF.uniform((B, 3, 32, 32), 7100).cuda()
    other = ((torch.arange(B) * 3 + 2) % G.K).cuda()
    with L.options(deterministic=1):
        mu, ls, la = model.encode(x)
        assert torch.equal(model.reconstruct(x, label=other), model.decode(mu, other, sigmoid=True))
        assert torch.equal(model.reconstruct(x), model.decode(mu, la.argmax(dim=1), sigmoid=True))
        # a posterior sample: z = mu + exp(ls) * n
        zs = dev_t(latent_z(5, 0, B, 128, mu.cpu().numpy(), ls.cpu().numpy()).astype(np.float32))
        assert terr(model.reconstruct(x, label=other, sample=True, key=5), model.decode(zs, other, sigmoid=True)) < FP32_TOL
    # against the CPU oracle's decoder
    lat = torch.cat([torch.from_numpy(z64.astype(np.float32)), torch.nn.functional.one_hot(labels.cpu(), G.K).float()], dim=1)
    with torch.no_grad():
        ref = torch.sigmoid(O.decoder_forward(state, lat[:, :, None, None], training=False, update=False))
    assert terr(img, ref) < FP32_TOL


def test_generate_k100():
    K, B, keyv = 100, 3, 42
    model, state = infer_model("wideresnet-10-1", K=K)
    labels = torch.tensor([99, 0, 57], device="cuda")
    img = model.generate(labels, keyv)
    z = latent_z(keyv, 0, B, 128).astype(np.float32)
    assert terr(img, torch.sigmoid(model.decode(dev_t(z), labels))) < FP32_TOL
    lat = torch.cat([torch.from_numpy(z), torch.nn.functional.one_hot(labels.cpu(), K).float()], dim=1)
    with torch.no_grad():
        ref = torch.sigmoid(O.decoder_forward(state, lat[:, :, None, None], training=False, update=False))
    e = terr(img, ref)
    print("FIG K=100 generate against the oracle's decoder: %.3e" % e)
    assert e < FP32_TOL
    x = CF.uniform((B, 3, 32, 32), 7100).cuda()
    assert tuple(model.encode(x)[2].shape) == (B, K) and int(model.predict(x).max()) < K


def _all_new_calls(model, x, labels):
    B = x.size(0)
    z = torch.zeros(B, 128, device="cuda")
    return [model.encode(x), model.features(x), model.predict(x), model.decode(z, labels), model.reconstruct(x),
            model.reconstruct(x, label=labels, sample=True, key=3), model.generate(labels, 9), model.generate(labels, 9, dtype="uint8"),
            model.feature_extractor(x), model.feature_reconstructor(torch.zeros(B, 128 + G.K, 1, 1, device="cuda"))]


def test_new_calls_leave_state_and_gradients_alone():
    model, _ = infer_model("wideresnet-10-1")
    x = CF.uniform((4, 3, 32, 32), 7100).cuda()
    labels = torch.tensor([1, 2, 3, 4], device="cuda")
    model.train()
    rec, mu, ls, la = model(x, disc_label=labels)           # a training forward + backward: gradients and counters are populated
    (rec.mean() + mu.mean() + ls.mean() + la.mean()).backward()
    model.eval()
    torch.cuda.synchronize()
    grad = model.flat_parameters()[1].clone()
    assert float(grad.abs().max()) > 0
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert all(int(v) == 1 for k, v in before.items() if k.endswith("num_batches_tracked"))
    outs = _all_new_calls(model, x, labels)
    torch.cuda.synchronize()
    for o in outs:
        for t in (o if isinstance(o, tuple) else (o,)):
            assert not t.requires_grad and t.grad_fn is None
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "a new call changed a parameter or a BatchNorm buffer"
    assert torch.equal(grad, model.flat_parameters()[1]), "a new call touched the gradients"
    assert not model._engine._pending
    assert all(p_.grad is not None for p_ in model.parameters())


def test_training_step_after_the_new_calls_equals_a_fresh_models():
    """with the unedited existing suite this holds Engine.forward, whose decoder loop moved into a helper, to its old behaviour"""
    name, K, Bl, Bu = "wideresnet-10-1", 10, 4, 6
    state = CF.make_state(name, K=K)
    il, ll, iu, lu = CF.make_batch(Bl, Bu, K)
    nz = CF.make_noise(Bl, Bu, K)
    sch = O.schedule(10)
    res = []
    with L.options(deterministic=1):
        for used in (False, True):
            model = make_model(name, K, "fp32", state)
            if used:
                model.eval()
                _all_new_calls(model, iu[:4].cuda(), ll.cuda())
                model.train()
            elbo, cls = S.VAECriterion(discrete_dim=K).cuda(), S.ClsCriterion()
            opt = S.FlatSGD(model)
            opt.zero_grad()
            with T.rng_for_step(nz):
                out = S.train_step(model, elbo, cls, opt, il.cuda(), ll.cuda(), iu.cuda(), sch, return_outputs=True)
            torch.cuda.synchronize()
            res.append((out, {k: v.clone() for k, v in model.state_dict().items()}))
    (o1, s1), (o2, s2) = res
    for k in T.SCALARS:
        assert float(o1[k]) == float(o2[k]), k
    for k in T.TENSORS:
        assert torch.equal(o1[k], o2[k]), k
    assert all(torch.equal(s1[k], s2[k]) for k in s1)


def _existing_eval_forward(model, x, eps, labels):
    """the existing eval forward with its context kept (forward_groups_direct): the four outputs, and the two intermediate tensors the
    new calls expose -- the pooled features (ctx.feat) and the encoder's output map, formed here in torch from the raw map the
    forward keeps (ctx.t[-1], NHWC) and the transition BatchNorm's running statistics + LeakyReLU (wideresnet.py:90-91)"""
    rec, mu, ls, la, ctx = model.forward_groups_direct([x], [dict(disc_label=labels)], eps.cuda(), None)
    sd = {k.replace(".module.", "."): v for k, v in model.state_dict().items()}
    pre = "feature_extractor.encoder.transition.norm."
    t = ctx.t[-1].float().permute(0, 3, 1, 2)
    fmap = torch.nn.functional.leaky_relu(torch.nn.functional.batch_norm(
        t, sd[pre + "running_mean"], sd[pre + "running_var"], sd[pre + "weight"], sd[pre + "bias"], False, 0.1, O.BN_EPS), O.LEAKY_SLOPE)
    return dict(rec=rec, sig=torch.sigmoid(rec), mu=mu, ls=ls, la=la, feat=ctx.feat, fmap=fmap)


def test_bf16_tracks_fp32():
    """Every new method once on wideresnet-28-2 in bf16 against the fp32 run of the same weights.  The new paths run the kernels of
    the eval model(x), so each output is gated by ITS OWN counterpart there: 2 x the bf16-vs-fp32 distance (max |a - b| / max |b|)
    of the same quantity of the existing eval forward on the same input, measured here -- mu / ls / la, the reconstruction's logits
    (decode, feature_reconstructor) and their sigmoid (reconstruct, generate, decode(sigmoid=True)) are its outputs; the pooled
    features and the encoder's output map are the tensors it keeps in its context.  uint8 pixels: one level more (both sides round).
    Measured on an MI355X (also in DESIGN.md 4b), existing forward: rec 3.8e-3, sigmoid(rec) 3.6e-4, mu 8.6e-4, ls 7.7e-4, la 4.9e-5,
    feat 1.6e-3, fmap 6.9e-3; new calls: encode 8.6e-4 / 7.7e-4 / 4.9e-5, features 1.6e-3, feature_extractor 6.9e-3, decode and
    feature_reconstructor 4.0e-3, the sigmoid images 3.4e-4 .. 4.0e-4."""
    name, B = "wideresnet-28-2", 8
    state = CF.make_state(name, K=G.K)
    m32, m16 = make_model(name, G.K, "fp32", state).eval(), make_model(name, G.K, "bf16", state).eval()
    x = CF.uniform((B, 3, 32, 32), 7100).cuda()
    eps = CF.normal((B, 128), 7101)
    labels = ((torch.arange(B) * 3 + 2) % G.K).cuda()
    e32, e16 = _existing_eval_forward(m32, x, eps, labels), _existing_eval_forward(m16, x, eps, labels)
    d = {k: terr(e16[k], e32[k]) for k in e32}
    print("FIG bf16 vs fp32, existing eval forward:", {k: "%.3e" % v for k, v in d.items()})
    assert all(0 < v < 0.1 for v in d.values())
    z = CF.normal((B, 128), 7102).cuda()
    soft = torch.softmax(CF.normal((B, G.K), 7103), dim=1).cuda()
    lat = torch.cat([z, soft], dim=1)[:, :, None, None].contiguous()
    calls = {"encode.mu": ("mu", lambda m: m.encode(x)[0]), "encode.ls": ("ls", lambda m: m.encode(x)[1]),
             "encode.la": ("la", lambda m: m.encode(x)[2]), "features": ("feat", lambda m: m.features(x)),
             "feature_extractor": ("fmap", lambda m: m.feature_extractor(x)),
             "decode": ("rec", lambda m: m.decode(z, labels)), "feature_reconstructor": ("rec", lambda m: m.feature_reconstructor(lat)),
             "decode soft": ("sig", lambda m: m.decode(z, soft, sigmoid=True)), "reconstruct": ("sig", lambda m: m.reconstruct(x)),
             "reconstruct swap": ("sig", lambda m: m.reconstruct(x, label=labels)),
             "reconstruct sample": ("sig", lambda m: m.reconstruct(x, label=labels, sample=True, key=4)),
             "generate": ("sig", lambda m: m.generate(labels, 11))}
    worst = []
    for k, (ref, fn) in calls.items():
        a, b = fn(m16), fn(m32)
        assert a.shape == b.shape and a.dtype == torch.float32
        e = terr(a, b)
        print("FIG bf16 vs fp32 %-22s %.3e  (allowed 2 x %s = %.3e)" % (k, e, ref, 2 * d[ref]))
        if e > 2 * d[ref]:
            worst.append((k, e, 2 * d[ref]))
    assert not worst, worst
    u16, u32 = m16.generate(labels, 11, dtype="uint8"), m32.generate(labels, 11, dtype="uint8")
    assert float((u16.float() - u32.float()).abs().max()) <= 255.0 * 2 * d["sig"] + 1.0
    assert torch.equal(m16.predict(x), m16.encode(x)[2].argmax(dim=1))


# B = 3 / 4: the output map (48 / 64 / 96 / 128 KB) is larger than the scratch's statistics block and no larger than that block and the
# coefficient block behind it together (36 + 40 KB on wideresnet-10-1, 92 + 99 KB on preactresnet18): a map placed on the freed
# scratch would cover the coefficients
@pytest.mark.parametrize("name,B", [("wideresnet-10-1", 1), ("wideresnet-10-1", 3), ("wideresnet-10-1", 4), ("wideresnet-10-1", 16),
                                    ("preactresnet18", 3), ("preactresnet18", 6), ("wideresnet-28-2", 33)])
def test_feature_extractor_at_other_batch_sizes_and_allocator_states(name, B):
    """feature_extractor's last launches read the eval forward's BatchNorm coefficients from its scratch: the scratch must outlive them.
    Batch sizes at which the output map is smaller / larger than that scratch, called on a fresh allocator cache, again (the cache
    now holds the first call's freed blocks, the scratch's among them) and after allocations of other sizes were made and freed;
    against the CPU oracle's encoder (held to the reference by tests/test_infer_cpu.py), and identical every time."""
    model, state = infer_model(name)
    x = CF.uniform((B, 3, 32, 32), 7200 + B)
    with P.patched(), torch.no_grad():
        want = O.encoder_forward(state, name, x, training=False, update=False)
    x = x.cuda()
    # the property itself, whatever the allocator does: the coefficients the later launches read lie in a buffer the context holds
    f, _, prot = model._engine._eval_encoder(x)
    lo = f.bnbuf.data_ptr()
    assert all(lo <= ptr < lo + f.bnbuf.numel() * 4 for ptr in prot[:2]), "the BatchNorm coefficients are not kept alive by the context"
    del f, prot
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    outs = [model.feature_extractor(x), model.feature_extractor(x)]
    junk = [torch.empty(n, device="cuda") for n in (1 << 10, 1 << 14, 3 << 14, 1 << 18, 5 << 16)]
    del junk
    outs.append(model.feature_extractor(x))
    outs.append(model.features(x))
    torch.cuda.synchronize()
    for i, o in enumerate(outs[:3]):
        e = terr(o, want)
        print("FIG %s B=%d feature_extractor call %d: %.3e" % (name, B, i, e))
        assert tuple(o.shape) == tuple(want.shape) and e < FP32_TOL, (i, e)
        assert torch.equal(o, outs[0]), "call %d differs from the first" % i
    assert terr(outs[3], want.mean(dim=(2, 3))) < FP32_TOL


def test_reconstruct_draws_its_own_key_like_a_dropout_key():
    """reconstruct(sample=True) without a key: one torch.randint draw from the host generator (rng="host"), the draw of a dropout key;
    it advances the generator, so two calls differ, and a call equals the one given that draw"""
    model, _ = infer_model("wideresnet-10-1")
    x = CF.uniform((4, 3, 32, 32), 7100).cuda()
    with L.options(deterministic=1):
        torch.manual_seed(123)
        a, b = model.reconstruct(x, sample=True), model.reconstruct(x, sample=True)
        torch.manual_seed(123)
        k1, k2 = (int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)) for _ in range(2))
        assert k1 != k2 and not torch.equal(a, b)
        assert torch.equal(a, model.reconstruct(x, sample=True, key=k1)) and torch.equal(b, model.reconstruct(x, sample=True, key=k2))
        assert not torch.equal(a, model.reconstruct(x))


def test_generate_under_graph_capture():
    """generate with a device key captured into a graph after one eager warm-up call, as GraphedStep does; replayed with another
    key written to the device it equals the eager call with that key"""
    model, _ = infer_model("wideresnet-10-1")
    B = 6
    labels = ((torch.arange(B) * 5 + 1) % G.K).cuda()
    key = torch.tensor([11], dtype=torch.int64, device="cuda")
    with L.options(deterministic=1):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            model.generate(labels, key, tau=0.9)                 # warm-up: weight packs and per-stream caches
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            out = model.generate(labels, key, tau=0.9)
        for k in (11, 12, 2 ** 40 + 5):
            key.fill_(k)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            want = model.generate(labels, key, tau=0.9)
            assert torch.equal(got, want), "replay with key %d differs from the eager call" % k
        assert not torch.equal(got, model.generate(labels, 11, tau=0.9))
