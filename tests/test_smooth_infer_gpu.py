"""Smooth-ELBO inference on a real MI355X.

Kernel level: sv_smooth_classify through the C ABI.  Its alpha must be BIT-equal to sv_smooth_latent_fwd's (training = 0) on the same
head output -- that kernel is held to float64 by tests/test_smooth_kernels_gpu.py, so no tolerance is needed here --, pred the first
maximum of the GPU's own alpha (numpy.argmax), -1 for the rows whose alpha holds a NaN, and the counters a numpy count, exactly.
Outputs are pre-filled (NaN / -7) and carry guard rows.

Model level, on the reference's fixtures (tests/golden/make_smooth_eval_goldens.py; allowances measured on the CPU by
tests/_smooth_infer.py, never from a GPU result): classify / evaluate_smooth / reconstruct against the fixtures, generate and traverse
against decode of explicitly built latents and the restated normal stream of tests/test_infer_cpu.py, and classify / generate under
graph capture.  bf16 reconstructions are gated at the 3e-2 of max-abs that tests/test_model_gpu.py sets for bf16 tensors.

Measured on an MI355X (svhn / mnist; max |a - ref| / max |ref| against the fixture, allowance in brackets): fp32 classify alpha 2.6e-6 /
2.9e-6 (about 1e-5; the allowances are measured when the test runs and move with the host CPU's fp32 summation: 1.1e-5 .. 1.3e-5 seen), reconstruct 1.9e-7 / 4.9e-7 (9.2e-7 / 2.3e-6), with a foreign label 1.9e-7 / 4.9e-7 (8.6e-7 / 2.9e-6),
decode 1.8e-7 / 3.5e-7 (1.1e-6 / 2.9e-6); bf16 alpha 1.6e-2 / 1.9e-2 (not gated: the predictions are), reconstructions 3.5e-3 ..
8.3e-3 (3e-2).  Undecided rows 14 / 41 of 256 at a top-2 gap of 0.31 / 0.38; on the decided rows no prediction differs from the
reference's in either mode, among the undecided ones bf16 flips one per kind (hits over all 256 rows: 170 / 171 against 170).
generate's z: 3.1e-7 of max |z| for the kernel and for the fp32 restatement alike; 12 rows drawn as 5 + 7 give the same bits, z and images."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _lib as L                              # noqa: E402
from oracle import smooth_oracle as SO                          # noqa: E402
from tests import _smooth_infer as SI                           # noqa: E402
from tests.golden import make_smooth_eval_goldens as G          # noqa: E402
from tests.test_infer_cpu import latent_normals                 # noqa: E402
from tests.test_smooth_kernels_gpu import DT, _latent_inputs, dev, gen, nan_like, p, pad16, st        # noqa: E402

BF16_TOL = 3e-2                  # tests/test_model_gpu.py: bf16 tensors, relative to the tensor's largest value
GUARD = 3
SHAPES = [(1, 32, 10), (7, 32, 100), (3, 70, 130), (261, 5, 3), (5, 4, 1)]


# ================================================================================================ sv_smooth_classify
def head_output(B, Dc, Dd, dt, seed, ties):
    """(o, labels, ldo) of tests/test_smooth_kernels_gpu.py's _latent_inputs: o = [mean | logvar | logits | pad (NaN: never read)] in
    the compute dtype, rows with tied maxima (some more than 64 positions apart).  That helper also plants six edge values in its
    uniform noise, which a case of fewer than six logits (B * Dd < 6) cannot hold; such a case gets the same o without the noise."""
    if B * Dd >= 6:
        o, _, _, label, ldo = _latent_inputs(B, Dc, Dd, dt, seed, ties)
        return o, label, ldo
    assert not ties
    g = gen(seed)
    ldo = pad16(2 * Dc + Dd)
    o = torch.full((B, ldo), float("nan"))
    o[:, :Dc] = torch.randn(B, Dc, generator=g)
    o[:, Dc:2 * Dc] = 0.7 * torch.randn(B, Dc, generator=g)
    o[:, 2 * Dc:2 * Dc + Dd] = 1.5 * torch.randn(B, Dd, generator=g)
    return o.to(DT[dt][1]), torch.randint(0, Dd, (B,), generator=g), ldo


def classify(dt, o, ldo, B, Dc, Dd, label=None, counts=None, confusion=None, want_alpha=True, want_pred=True):
    """one call into pre-filled outputs with GUARD rows behind them -> (alpha [B, Dd] numpy or None, pred [B] numpy or None)"""
    alpha = nan_like((B + GUARD, Dd), torch.float32) if want_alpha else None
    pred = torch.full((B + GUARD,), -7, dtype=torch.int64, device=dev()) if want_pred else None
    L.call("sv_smooth_classify", DT[dt][0], p(o), ldo, B, Dc, Dd, p(label), p(alpha), p(pred), p(counts), p(confusion), st())
    torch.cuda.synchronize()
    if want_alpha:
        assert torch.isnan(alpha[B:]).all(), "alpha: guard rows written"
    if want_pred:
        assert bool((pred[B:] == -7).all()), "pred: guard rows written"
    return (alpha[:B].cpu().numpy() if want_alpha else None), (pred[:B].cpu().numpy() if want_pred else None)


def latent_fwd_alpha(dt, o, ldo, B, Dc, Dd):
    """alpha and the eval-mode one-hot of sv_smooth_latent_fwd (training = 0, no label) on the same head output"""
    code, tdt = DT[dt]
    Lpad = pad16(Dc + Dd)
    f32 = lambda *s: nan_like(s, torch.float32)
    mean, logvar, alpha, gs, l32 = f32(B, Dc), f32(B, Dc), f32(B, Dd), f32(B, Dd), f32(B, Dc + Dd)
    lat = nan_like((B, Lpad), tdt)
    L.call("sv_smooth_latent_fwd", code, p(o), ldo, None, None, None, 0.67, 0, B, Dc, Dd, Lpad, p(mean), p(logvar), p(alpha), p(gs),
           p(lat), p(l32), st())
    torch.cuda.synchronize()
    return alpha.cpu().numpy(), gs.cpu().numpy()


def count_ref(pred, label, Dd):
    """(hits, rows, confusion) as numpy counts them: a label outside [0, Dd) or a pred of -1 is a miss and in no cell"""
    conf = np.zeros((Dd, Dd), dtype=np.int64)
    ok = (label >= 0) & (label < Dd) & (pred >= 0)
    np.add.at(conf, (label[ok], pred[ok]), 1)
    return int((pred == label)[pred >= 0].sum()), len(pred), conf


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("B,Dc,Dd", SHAPES)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_smooth_classify_kernel(dt, B, Dc, Dd):
    d = dev()
    o, label, ldo = head_output(B, Dc, Dd, dt, 31 + B + Dd, ties=Dd >= 3)
    od = o.to(d)
    want_alpha, _ = latent_fwd_alpha(dt, od, ldo, B, Dc, Dd)
    alpha, pred = classify(dt, od, ldo, B, Dc, Dd)
    assert np.isfinite(alpha).all() and np.array_equal(bits(alpha), bits(want_alpha)), "alpha is not bit-equal to sv_smooth_latent_fwd's"
    assert np.array_equal(pred, alpha.argmax(1)), "pred is not the first maximum of alpha"
    if Dd > 64:
        assert pred[1] == 3 and pred[B - 1] == 5                  # tied maxima more than 64 positions apart: the first one
    # counters: labels made of the predictions (hits), other classes, and values outside [0, Dd)
    g = torch.Generator().manual_seed(5 + B)
    lab = torch.from_numpy(pred).clone()
    other = torch.rand(B, generator=g) < 0.4
    lab[other] = label[other]
    if B > 4:
        lab[1], lab[3], lab[B - 1] = -1, Dd, 2 ** 40
    else:
        lab[B - 1] = Dd
    lab2 = torch.roll(lab, 1)
    counts = torch.zeros(2, dtype=torch.int64, device=d)
    conf = torch.zeros(Dd, Dd, dtype=torch.int64, device=d)
    h1, n1, c1 = count_ref(pred, lab.numpy(), Dd)
    h2, n2, c2 = count_ref(pred, lab2.numpy(), Dd)
    a1, p1 = classify(dt, od, ldo, B, Dc, Dd, lab.to(d), counts, conf)
    assert counts.tolist() == [h1, n1] and np.array_equal(conf.cpu().numpy(), c1)
    assert np.array_equal(bits(a1), bits(alpha)) and np.array_equal(p1, pred)
    classify(dt, od, ldo, B, Dc, Dd, lab2.to(d), counts, conf)               # a second call accumulates
    assert counts.tolist() == [h1 + h2, n1 + n2] and np.array_equal(conf.cpu().numpy(), c1 + c2)
    # each output NULL in turn: the others are what they were
    for skip in ("alpha", "pred", "confusion", "counts"):
        counts.zero_()
        conf.zero_()
        a, q = classify(dt, od, ldo, B, Dc, Dd, lab.to(d), None if skip == "counts" else counts, None if skip == "confusion" else conf,
                        want_alpha=skip != "alpha", want_pred=skip != "pred")
        assert a is None or np.array_equal(bits(a), bits(alpha)), skip
        assert q is None or np.array_equal(q, pred), skip
        assert counts.tolist() == ([0, 0] if skip == "counts" else [h1, n1]), skip
        assert np.array_equal(conf.cpu().numpy(), 0 * c1 if skip == "confusion" else c1), skip
    a, q = classify(dt, od, ldo, B, Dc, Dd, want_pred=False)                 # alpha alone, no labels
    assert q is None and np.array_equal(bits(a), bits(alpha))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_smooth_classify_rows_without_a_prediction(dt):
    """a NaN logit, a +inf logit and all logits -inf make the row's alpha NaN (the arithmetic of sv_smooth_latent_fwd, whose eval-mode
    one-hot is all zero there): pred = -1, a miss that is in no cell of the confusion matrix; -inf beside finite logits is a zero"""
    B, Dc, Dd = 7, 4, 70
    d = dev()
    o, _, ldo = head_output(B, Dc, Dd, dt, 77, ties=False)
    o = o.float()
    inf = float("inf")
    o[0, 2 * Dc + 69] = float("nan")
    o[2, 2 * Dc + 1] = inf
    o[4, 2 * Dc:2 * Dc + Dd] = -inf
    o[5, 2 * Dc:2 * Dc + Dd] = -inf
    o[5, 2 * Dc + 66] = 0.5                                   # one finite logit: alpha = its one-hot
    o[6, 2 * Dc + 3] = -inf
    od = o.to(DT[dt][1]).to(d)
    want_alpha, want_gs = latent_fwd_alpha(dt, od, ldo, B, Dc, Dd)
    label = torch.tensor([1, 2, 1, 4, 0, 66, 9], dtype=torch.int64)
    counts = torch.zeros(2, dtype=torch.int64, device=d)
    conf = torch.zeros(Dd, Dd, dtype=torch.int64, device=d)
    alpha_t = torch.full((B, Dd), 3.0, device=d)
    pred_t = torch.full((B,), -7, dtype=torch.int64, device=d)
    L.call("sv_smooth_classify", DT[dt][0], p(od), ldo, B, Dc, Dd, p(label.to(d)), p(alpha_t), p(pred_t), p(counts), p(conf), st())
    torch.cuda.synchronize()
    alpha, pred = alpha_t.cpu().numpy(), pred_t.cpu().numpy()
    assert np.array_equal(alpha, want_alpha, equal_nan=True)
    bad = [0, 2, 4]
    assert np.isnan(alpha[bad]).all() and (want_gs[bad] == 0).all() and np.isfinite(np.delete(alpha, bad, axis=0)).all()
    assert (pred[bad] == -1).all() and pred[5] == 66 and alpha[5, 66] == 1.0 and alpha[6, 3] == 0.0
    good = np.array([1, 3, 5, 6])
    assert np.array_equal(pred[good], alpha[good].argmax(1))
    h, n, c = count_ref(pred, label.numpy(), Dd)
    assert counts.tolist() == [h, n] == [int((pred[good] == label.numpy()[good]).sum()), B]
    assert np.array_equal(conf.cpu().numpy(), c) and int(c.sum()) == len(good)


# ================================================================================================ model level
_MODELS = {}


def model_for(kind, dtype, train=True):
    """the fixture's model on the GPU, made once per (kind, dtype); left in training mode: nothing here needs eval()"""
    m = _MODELS.get((kind, dtype))
    if m is None:
        m = S.SmoothVAE((SO.KINDS[kind]["in_ch"], 32, 32), {"cont": G.CONT, "disc": [G.DISC]}, temperature=0.67, compute_dtype=dtype)
        m.load_state_dict(SI.case(kind)["st"])
        m = _MODELS[(kind, dtype)] = m.cuda()
    return m.train(train)


def terr(t, ref):
    return SI.rel(t.detach().float().cpu(), ref)


CASES = [(k, dt) for k in G.KINDS for dt in ("fp32", "bf16")]


@pytest.mark.parametrize("kind,dtype", CASES)
def test_classify_matches_the_reference(kind, dtype):
    c = SI.case(kind)
    g, decided = c["g"], c["decided"]
    m = model_for(kind, dtype)
    x = c["x"].cuda()
    alpha, pred = m.classify(x)
    assert tuple(alpha.shape) == (256, 10) and alpha.dtype == torch.float32 and pred.dtype == torch.int64
    assert not alpha.requires_grad and m.training, "classify leaves no autograd history and the mode alone"
    assert torch.equal(pred, alpha.argmax(1)) and torch.equal(m.predict(x), pred)
    e = terr(alpha, g["alpha"])
    print("FIG %s %s classify alpha against the fixture %.3e (fp32 allowance %.3e); undecided rows %d, gap %.4f"
          % (kind, dtype, e, c["tol_alpha"], int((~decided).sum()), c["gap"]))
    assert int((~decided).sum()) <= SI.MAX_UNDECIDED
    if dtype == "fp32":
        assert e <= c["tol_alpha"], (kind, e, c["tol_alpha"])
    wrong = int((pred.cpu().numpy() != g["pred"])[decided].sum())
    print("FIG %s %s predictions that differ from the fixture: %d decided, %d undecided"
          % (kind, dtype, wrong, int((pred.cpu().numpy() != g["pred"])[~decided].sum())))
    assert wrong == 0
    # the same alpha as the forward's, bit for bit, in either mode
    with torch.no_grad():
        fa = m(x)[1]["disc"][0]
    assert torch.equal(fa, alpha)
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x)[1]["disc"][0], alpha)
    m.train()


@pytest.mark.parametrize("kind,dtype", CASES)
def test_evaluate_smooth_counts_what_the_reference_counts(kind, dtype):
    c = SI.case(kind)
    g, decided = c["g"], c["decided"]
    m = model_for(kind, dtype)
    idx = torch.from_numpy(np.nonzero(decided)[0])
    x, y = c["x"][idx].cuda(), c["label"][idx].cuda()
    want_hits = int((g["pred"] == g["label"])[decided].sum())
    want_conf = confusion_ref(g["label"][decided], g["pred"][decided])
    n = x.shape[0]
    for parts in ([slice(0, 100), slice(100, 200), slice(200, n)], [slice(0, n)]):
        r = S.evaluate_smooth(m, [(x[s], y[s]) for s in parts])
        assert (r["correct"], r["total"]) == (want_hits, n) and r["accuracy"] == want_hits / n
        assert np.array_equal(r["confusion"], want_conf) and r["confusion"].dtype == np.int64
        rows = want_conf.sum(1)
        assert np.allclose(r["per_class_accuracy"][rows > 0], (np.diag(want_conf) / np.maximum(rows, 1))[rows > 0])
        assert np.isnan(r["per_class_accuracy"][rows == 0]).all()
    # all 256 rows: only an undecided row may be counted differently
    r = S.evaluate_smooth(m, [(c["x"][:100].cuda(), c["label"][:100].cuda()), (c["x"][100:].cuda(), c["label"][100:].cuda())])
    print("FIG %s %s hits over all 256 rows: %d, the fixture's %d (undecided %d)" % (kind, dtype, r["correct"], int(g["hits"]),
                                                                                    int((~decided).sum())))
    assert r["total"] == 256 and abs(r["correct"] - int(g["hits"])) <= int((~decided).sum())
    # the evaluator object: reset() starts over, update() returns the batch's predictions
    ev = S.SmoothEvaluator(m)
    ev.update(x[:7], y[:7])
    ev.reset()
    pr = ev.update(x, y)
    assert np.array_equal(pr.cpu().numpy(), g["pred"][decided]) and ev.result()["correct"] == want_hits


def confusion_ref(label, pred, Dd=G.DISC):
    conf = np.zeros((Dd, Dd), dtype=np.int64)
    np.add.at(conf, (label, pred), 1)
    return conf


@pytest.mark.parametrize("kind,dtype", CASES)
def test_reconstruct_matches_the_reference(kind, dtype):
    c = SI.case(kind)
    g, n = c["g"], G.N_REC
    m = model_for(kind, dtype)
    x, foreign = c["x"][:n].cuda(), c["foreign"].cuda()
    rec, rec_label = m.reconstruct(x), m.reconstruct(x, foreign)
    assert tuple(rec.shape) == g["rec"].shape and rec.dtype == torch.float32 and not rec.requires_grad and m.training
    # under the predicted class a flipped argmax is another image: bf16 is held on the decided rows (their class is pinned); fp32
    # on all of them -- its logit error is some 1e-5, four orders below the smallest top-2 gap of these rows (0.09)
    dec = torch.arange(n) if dtype == "fp32" else torch.from_numpy(np.nonzero(c["decided"][:n])[0])
    assert len(dec) >= n // 2
    e1, e2 = terr(rec[dec.cuda()], g["rec"][dec.numpy()]), terr(rec_label, g["rec_label"])
    e3 = terr(m.decode(c["latent"].cuda()).detach(), g["rec_latent"])
    print("FIG %s %s reconstruct %.3e (allow %.3e), with a foreign label %.3e (allow %.3e), decode %.3e (allow %.3e); decided %d of %d"
          % (kind, dtype, e1, c["tol_rec"], e2, c["tol_rec_label"], e3, c["tol_rec_latent"], len(dec), n))
    lim = (c["tol_rec"], c["tol_rec_label"], c["tol_rec_latent"]) if dtype == "fp32" else (BF16_TOL,) * 3
    assert e1 <= lim[0] and e2 <= lim[1] and e3 <= lim[2], (kind, dtype, e1, e2, e3, lim)
    # the eval-mode forward's reconstruction, bit for bit, with the module left in training mode
    m.eval()
    with torch.no_grad():
        want, want_label = m(x)[0], m(x, foreign)[0]
    m.train()
    assert torch.equal(m.reconstruct(x), want) and torch.equal(m.reconstruct(x, foreign), want_label)
    assert torch.equal(rec, want) and torch.equal(rec_label, want_label) and m.training


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_generate_is_decode_of_the_restated_stream(dtype):
    kind, B, keyv, tau = "svhn", 12, 987654321012345, 0.8
    m = model_for(kind, dtype)
    Dc, Dd = m.latent_cont_dim, m.latent_disc_dim
    label = ((torch.arange(B) * 5 + 1) % Dd).cuda()
    img, z = m.generate(label, keyv, tau=tau, return_z=True)
    assert tuple(img.shape) == (B, 3, 32, 32) and img.dtype == torch.float32 and not img.requires_grad
    assert tuple(z.shape) == (B, Dc) and z.dtype == torch.float32
    assert float(img.abs().max()) <= 1.0
    with torch.no_grad():
        want = m.decode(torch.cat([z, F.one_hot(label, Dd).float()], dim=1))
    assert torch.equal(img, want), "generate != decode(cat[z, one-hot])"
    assert torch.equal(m.generate(label, keyv, tau=tau), img)
    # z = tau * n(row0 + b, d) of sv_latent_draw's stream: 8 x the fp32 restatement's error against the float64 one
    tau32 = np.float64(np.float32(tau))
    z64 = tau32 * latent_normals(keyv, 0, B, Dc)
    z32 = np.float32(tau) * latent_normals(keyv, 0, B, Dc, np.float32)
    cpu, e = SI.rel(z32, z64), SI.rel(z.cpu().numpy(), z64)
    print("FIG %s generate z: cpu32 %.3e kernel %.3e" % (dtype, cpu, e))
    assert e <= 8.0 * max(cpu, SI.HALF_ULP)
    # rows row0 .. row0 + B - 1 in one call = the same rows in two calls; a device key = the int
    key = torch.tensor([keyv], dtype=torch.int64, device="cuda")
    a, za = m.generate(label[:5], key, tau=tau, return_z=True)
    b, zb = m.generate(label[5:], key, row0=5, tau=tau, return_z=True)
    assert torch.equal(torch.cat([za, zb]), z), "z of rows 0 .. 11 drawn as 5 + 7 differs from one call's"
    # ... and so do the images, bit for bit: what generate's docstring promises of a row (its z AND its image)
    assert torch.equal(torch.cat([a, b]), img), "images of rows 0 .. 11 drawn as 5 + 7 differ from one call's"
    assert not torch.equal(m.generate(label, keyv + 1, tau=tau), img)
    zoff = m.generate(label, key, row0=2 ** 33, tau=tau, return_z=True)[1]          # a row index beyond 2^32
    assert SI.rel(zoff.cpu().numpy(), tau32 * latent_normals(keyv, 2 ** 33, B, Dc)) <= 8.0 * max(cpu, SI.HALF_ULP)


@pytest.mark.parametrize("kind,dtype", [("svhn", "fp32"), ("mnist", "bf16")])
def test_traverse_is_decode_of_the_built_latents(kind, dtype):
    m = model_for(kind, dtype)
    Dc, Dd, ch = m.latent_cont_dim, m.latent_disc_dim, SO.KINDS[kind]["in_ch"]
    B = 3
    z = torch.from_numpy(latent_normals(4, 0, B, Dc, np.float32)).cuda()
    label = torch.tensor([7, 0, 3], device="cuda")
    values = [-2.0, -0.5, 0.0, 1.25, 3.0]
    out = m.traverse(z, label, dim=5, values=values)
    assert tuple(out.shape) == (B, len(values), ch, 32, 32) and out.dtype == torch.float32 and not out.requires_grad
    rows = []
    for b in range(B):
        for v in values:
            zz = z[b].clone()
            zz[5] = v
            rows.append(torch.cat([zz, F.one_hot(label[b], Dd).float()]))
    with torch.no_grad():
        want = m.decode(torch.stack(rows))
    assert torch.equal(out.flatten(0, 1), want)
    assert torch.equal(m.traverse(z, label, dim=5, values=torch.tensor(values, device="cuda")), out)
    sweep = m.traverse(z, label)
    assert tuple(sweep.shape) == (B, Dd, ch, 32, 32)
    rows = [torch.cat([z[b], F.one_hot(torch.tensor(k, device="cuda"), Dd).float()]) for b in range(B) for k in range(Dd)]
    with torch.no_grad():
        assert torch.equal(sweep.flatten(0, 1), m.decode(torch.stack(rows)))
    assert not torch.equal(sweep[0, 0], sweep[0, 1])


# ================================================================================================ graph capture
def _capture(body):
    """warm-up on a side stream, then one capture of body() on it (the pattern of GraphedSmoothStep) -> (graph, body's result)"""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        body()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        out = body()
    return graph, out


def test_classify_with_counts_is_capturable():
    kind = "svhn"
    c = SI.case(kind)
    m = model_for(kind, "bf16")
    x1, y1 = c["x"][:64].cuda(), c["label"][:64].cuda()
    x2, y2 = c["x"][64:128].cuda(), c["label"][64:128].cuda()
    eager = torch.zeros(2, dtype=torch.int64, device="cuda")
    p1 = m.classify(x1, y1, eager)[1].clone()
    p2 = m.classify(x2, y2, eager)[1].clone()
    xs, ys = x1.clone(), y1.clone()
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    graph, (_, pred) = _capture(lambda: m.classify(xs, ys, counts))
    counts.zero_()                                        # (the warm-up call counted; the capture itself runs nothing)
    xs.copy_(x1)
    ys.copy_(y1)
    graph.replay()
    assert torch.equal(pred, p1)
    xs.copy_(x2)
    ys.copy_(y2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(pred, p2) and counts.tolist() == eager.tolist() and counts[1].item() == 128


def test_generate_is_capturable_with_a_device_key():
    m = model_for("svhn", "bf16")
    label = ((torch.arange(16) * 3) % m.latent_disc_dim).cuda()
    key = torch.tensor([11], dtype=torch.int64, device="cuda")
    graph, img = _capture(lambda: m.generate(label, key, tau=0.9))
    for k in (11, 12345678901):
        key.fill_(k)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(img, m.generate(label, k, tau=0.9)), k
