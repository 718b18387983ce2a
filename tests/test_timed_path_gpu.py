"""The path bench.py TIMES, under test at the sizes it is timed at (round-2 verdict, item 1).

bench.py's default step is `train_step_grouped` through the engine's DEFAULT state: the four forwards of
main_shot_vae.py:280-366 as one batched launch sequence (groups = 4), the weight gradients on a side stream, the body
convolutions' weight / data gradient pairs with half the persistent-block budget each.  Here that step runs at BASELINE
config 2 (WRN-28-2, K = 10, B_l = B_u = 512) and config 4 (WRN-28-10, K = 100, B_l = B_u = 256) in bf16, ten times from the
same state next to a stream that saturates HBM, against (a) the sequential step on identical scripted noise (loss terms,
BatchNorm running statistics, gradient direction), (b) its own first repeat and (c) the fp32 CPU oracle's loss terms.
Kernel level: conv3x3x / conv3x3p forward + data gradient with groups = 4 against four separate launches (bit for bit) and
the wide / narrow 3x3 weight gradients with groups = 4 against the sum of four launches, at 4 x 256 ... 4 x 512 images.
One svhn_VAE iteration at BASELINE config 5's per-GPU size (B_u = B_l = 1024, main_smooth_ELBO_svhn.py:228-388)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                     # noqa: E402
from oracle import shotvae_oracle as O       # noqa: E402
from shot_vae_amd import _lib as L           # noqa: E402
from shot_vae_amd import geometry as G       # noqa: E402
from tests import _cases as T                # noqa: E402
from tests.test_wide_gpu import _HbmLoad, _conv_args, _st      # noqa: E402

BF = torch.bfloat16


def _model(name, K, init):
    m = S.VariationalAutoEncoder(name, num_input_channels=3, img_size=(32, 32), data_parallel=True,
                                 continuous_latent_dim=128, disc_latent_dim=K, small_input=True, compute_dtype="bf16")
    m.load_state_dict({k: v.detach() for k, v in init.items()})
    return m.cuda().train()


def _running(model):
    return {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items() if "running_" in k}


@pytest.mark.parametrize("name,K,B,dmi,tol", [("wideresnet-28-2", 10, 512, 2.3, 5e-3), ("wideresnet-28-10", 100, 256, 4.6, 5e-3)])
def test_grouped_step_default_engine_state_at_full_size(name, K, B, dmi, tol):
    torch.manual_seed(17)
    il, ll, iu = torch.rand(B, 3, 32, 32), torch.randint(0, K, (B,)), torch.rand(B, 3, 32, 32)
    nz = O.make_noise(B, B, K, seed=23)
    nz["lam_l"] = 0.9                      # Beta(0.1, 0.1) draws sit at 0 or 1: keep the mixed forward non-degenerate
    sch = O.schedule(10, dmi=dmi)
    init = O.default_init(name, K=K, seed=5)
    elbo, cls = S.VAECriterion(discrete_dim=K, bce_reconstruction=True).cuda(), S.ClsCriterion()
    ilc, llc, iuc = il.cuda(), ll.cuda(), iu.cuda()

    # (a) the sequential step (reference order, one launch sequence per forward) from the same state
    seq = _model(name, K, init)
    S.FlatSGD(seq).zero_grad()
    with T.rng_for_step(nz):
        ref = S.train_step(seq, elbo, cls, None, ilc, llc, iuc, sch, return_outputs=True)
    torch.cuda.synchronize()
    g_seq = seq.flat_parameters()[1].detach().double().clone()
    run_seq = _running(seq)
    ref = {k: float(ref[k]) for k in T.SCALARS}
    del seq

    # the timed path: default engine state = side stream on, paired block budgets
    model = _model(name, K, init)
    eng = model._engine
    assert eng.wgrad_side_stream and eng.pair_blocks == 256, "this test must run the engine's DEFAULT state"
    opt = S.FlatSGD(model)
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    load = _HbmLoad()
    first, g0, worst_cos, all_vals = None, None, 1.0, []
    for rep in range(10):
        model.load_state_dict(state0)          # same parameters AND running statistics every repeat
        opt.zero_grad()
        if rep % 3 == 1:
            load.kick(8)
        with T.rng_for_step(nz):
            out = S.train_step_grouped(model, elbo, cls, None, ilc, llc, iuc, sch, return_outputs=True)
        torch.cuda.synchronize()
        vals = {k: float(out[k]) for k in T.SCALARS}
        all_vals.append(vals)
        grad = model.flat_parameters()[1].detach().double().clone()
        assert all(np.isfinite(v) for v in vals.values()), (rep, vals)
        assert bool(torch.isfinite(grad).all()), rep
        if rep == 0:
            first, g0 = vals, grad
            for i in (1, 2, 3, 4):                       # size-independent properties
                la = out["la%d" % i].double()
                assert float((la.exp().sum(1) - 1).abs().max()) < 1e-5
            for i in (1, 3):                             # (rec2 / rec4 enter no loss term and are not computed)
                assert out["rec%d" % i].shape == (B, 3, 32, 32) and bool(torch.isfinite(out["rec%d" % i]).all())
            mu, lsg = out["mu1"].double(), out["ls1"].double()
            klc = 0.5 * (mu * mu + torch.exp(2 * lsg) - 2 * lsg - 1).sum() / B
            assert abs(float(klc) - vals["klc_l"]) < 1e-3 * float(klc)
            assert 0.0 <= vals["kld_l"] <= np.log(K) + 1e-4
            # grouped = sequential: the batched kernels see exactly the per-forward problems
            wseq = max(abs(vals[k] - ref[k]) / max(abs(ref[k]), 1e-6) / (2 if "_post_" in k else 1) for k in T.SCALARS)
            print("\n[%s B=%d] grouped vs sequential: worst loss-scalar deviation %.2e of the gate unit (gate %.0e)" % (name, B, wseq, tol))
            for k in T.SCALARS:
                tk = 2 * tol if "_post_" in k else tol
                assert abs(vals[k] - ref[k]) <= tk * max(abs(ref[k]), 1e-6), ("grouped vs sequential", k, vals[k], ref[k])
            cos = float(grad @ g_seq / grad.norm() / g_seq.norm())
            print("\n[%s B=%d] grouped vs sequential: flat-gradient cosine %.4f" % (name, B, cos))
            # (TWO DIFFERENT SUMMATION TREES of the same BatchNorm statistics -- one launch of four groups against four launches
            #  partition the pixels over the blocks differently -- i.e. two valid fp32 roundings of the same sums, 1e-7 apart: the
            #  bf16 step at its initial weights amplifies that to ~2 % of the gradient (0.983 at config 2, 1.0000 at config 4,
            #  measured).  Repeats of ONE schedule, below, agree to fp32 rounding since the accumulators are doubles.)
            assert cos > 0.95, cos
            run = _running(model)
            for k in run_seq:
                assert T.rel_err(run[k].numpy(), run_seq[k].numpy()) < 2e-2, k
            nbt = [int(v) for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")]
            assert set(nbt) == {4}
        else:
            cos = float(grad @ g0 / grad.norm() / g0.norm())
            worst_cos = min(worst_cos, cos)
            assert cos > 0.9999, (rep, cos)   # (rounds 3-4: 0.968 - 0.983 against the first run -- fp32 statistic atomics)
    print("[%s B=%d] 10 repeats of the timed path: lowest gradient cosine against the first %.4f" % (name, B, worst_cos))
    # the same step ten times: only the order of the float atomics may differ -- every run within the spread of the MEDIAN run
    # (a single reference run may itself be the outlier; the posterior terms are differences between the outputs of two
    # forwards: twice the spread, as everywhere)
    med = {k: sorted(v[k] for v in all_vals)[len(all_vals) // 2] for k in all_vals[0]}
    for rep, v in enumerate(all_vals):
        for k in v:
            tk = 4e-4 if "_post_" in k else 2e-4
            assert abs(v[k] - med[k]) <= tk * max(abs(med[k]), 1e-3), (rep, k, v[k], med[k])
    # (c) loss terms against the fp32 CPU oracle on the same inputs and noise -- and at config 2 the oracle's BACKWARD too
    #     (main_shot_vae.py:324,364): the full-size gradient is held to the reference's arithmetic, not only to the sequential
    #     HIP step (the larger network costs minutes of host time per backward and stays with the forward)
    st = {k: v.clone() for k, v in init.items()}
    with_grad = name == "wideresnet-28-2"
    if with_grad:
        for k in st:
            if O.is_param(k):
                st[k].requires_grad_(True)
        orc = O.train_step(st, name, il, ll, iu, nz, sch)
        model.load_state_dict(state0)
        fa, fb, ratios = [], [], {}
        sdg = {k.replace(".module.", "."): p for k, p in model.named_parameters()}
        # g0 is the flat buffer of the first repeat; its per-tensor views follow the module's parameters
        opt.zero_grad()
        model.flat_parameters()[1].copy_(g0.float())
        for k in st:
            if not O.is_param(k) or k.endswith("conv0.bias"):      # conv0.bias: analytically zero gradient
                continue
            a_, b_ = sdg[k].grad.detach().double().cpu().flatten(), st[k].grad.double().flatten()
            fa.append(a_)
            fb.append(b_)
            ratios[k] = float(a_.norm() / b_.norm().clamp_min(1e-30))
        fa, fb = torch.cat(fa), torch.cat(fb)
        cos_o = float(fa @ fb / fa.norm() / fb.norm())
        grel_o = float((fa - fb).norm() / fb.norm())
        big = {k: r for k, r in ratios.items() if "weight" in k and "norm" not in k and ".bias" not in k}
        print("[%s B=%d] first repeat vs fp32 oracle GRADIENT: flat cosine %.4f, relative L2 %.3f, conv / linear weight norm "
              "ratios %.3f .. %.3f" % (name, B, cos_o, grel_o, min(big.values()), max(big.values())))
        # bf16 operands against fp32 arithmetic on an ill-conditioned step: torch's own bf16 autocast of the oracle reaches
        # cosine 0.914 / relative L2 0.416 at B = 64; the full-size HIP step must do at least as well
        assert cos_o > 0.914 and grel_o < 0.416, (cos_o, grel_o)
        assert 0.8 < min(big.values()) and max(big.values()) < 1.25, sorted(big.items(), key=lambda kv: kv[1])[:3]
    else:
        with torch.no_grad():
            orc = O.train_step(st, name, il, ll, iu, nz, sch, backward=False)
    worc = max(abs(med[k] - float(orc[k])) / max(abs(float(orc[k])), 1e-6) / (2 if "_post_" in k else 1) for k in T.SCALARS)
    print("[%s B=%d] median run vs fp32 oracle: worst loss-scalar deviation %.2e of the gate unit (gate %.0e)" % (name, B, worc, tol))
    for k in T.SCALARS:
        r = float(orc[k])
        tk = 2 * tol if "_post_" in k else tol
        assert abs(med[k] - r) <= tk * max(abs(r), 1e-6), ("median run vs fp32 oracle", k, med[k], r)


# Cin, H, N, images per group: the WRN-28-10 body at config 4's grouped size and the WRN-28-2 body at config 2's
FWD_SHAPES = [(160, 32, 160, 256), (320, 16, 320, 256), (640, 8, 640, 256), (32, 32, 32, 512), (64, 16, 64, 512),
              (128, 8, 128, 512)]


@pytest.mark.parametrize("Cin,H,N,B", FWD_SHAPES)
def test_groups4_forward_and_dgrad_bitwise_at_full_size(Cin, H, N, B):
    """sv_igemm with groups = 4 through the DEFAULT dispatch (conv3x3x: one item queue across the group boundaries;
    conv3x3p / conv3x3w: persistent blocks shared among the groups) against four separate launches: outputs bit for
    bit, the per-group statistics to summation order.  Both block budgets the step uses (512, and 256 = paired)."""
    Gn, d = 4, torch.device("cuda:0")
    torch.manual_seed(Cin + H)
    load = _HbmLoad()
    master = (torch.randn(N, 9, Cin, device=d) / (9 * Cin) ** 0.5).contiguous()
    gf = G.conv_like(B, H, H, Cin, N, 3, 1, 1)
    gd = G.convT_like(B, H, H, N, Cin, 3, 1, 1)
    wf = torch.zeros(G.packed_size(gf), dtype=BF, device=d)
    wd = torch.zeros(G.packed_size(gd), dtype=BF, device=d)
    L.call("sv_repack", L.SV_BF16, C.c_void_p(master.data_ptr()), N, 9, Cin, 0, C.byref(gf), C.c_void_p(wf.data_ptr()), _st())
    L.call("sv_repack", L.SV_BF16, C.c_void_p(master.data_ptr()), N, 9, Cin, 1, C.byref(gd), C.c_void_p(wd.data_ptr()), _st())
    R = 8
    for budget in (512, 256):
        x = torch.randn(Gn * B, H, H, Cin, device=d).to(BF)
        resid = torch.randn(Gn * B, H, H, N, device=d).to(BF)
        dy = torch.randn(Gn * B, H, H, N, device=d).to(BF)
        sc, sh = (torch.rand(Gn, Cin, device=d) + 0.5).contiguous(), (torch.randn(Gn, Cin, device=d) * 0.3).contiguous()
        emu, ers = (torch.randn(Gn, Cin, device=d) * 0.1).contiguous(), (torch.rand(Gn, Cin, device=d) + 0.5).contiguous()

        def run(sl, gi, groups):
            xs, rs, dys = x[sl], resid[sl], dy[sl]
            v = (lambda t: t if gi is None else t[gi].contiguous())
            out = torch.zeros(xs.shape[0], H, H, N, dtype=BF, device=d)
            stats = torch.zeros(groups, R, 2 * N, device=d, dtype=torch.float64)        # sv_acc_t
            a = _conv_args(xs, wf, out, v(sc), v(sh), resid=rs, stats=stats)
            a.replicas, a.groups = R, groups
            L.call("sv_igemm", C.byref(gf), L.SV_BF16, C.byref(a), _st())
            dx = torch.zeros(xs.shape[0], H, H, Cin, dtype=BF, device=d)
            bs = torch.zeros(groups, R, 2 * Cin, device=d, dtype=torch.float64)
            a2 = _conv_args(dys, wd, dx, None, None, ex=(xs, v(sc), v(sh), v(emu), v(ers), bs))
            a2.replicas, a2.groups = R, groups
            L.call("sv_igemm", C.byref(gd), L.SV_BF16, C.byref(a2), _st())
            torch.cuda.synchronize()
            return out, stats.sum(1), dx, bs.sum(1)

        with L.options(persistent_blocks=budget):
            load.kick()
            ob, sb, db, bb = run(slice(None), None, Gn)
            assert bool(torch.isfinite(ob.float()).all()) and bool(torch.isfinite(db.float()).all())
            for gi in range(Gn):
                sl = slice(gi * B, (gi + 1) * B)
                o1, s1, d1, b1 = run(sl, gi, 1)
                nf = int((ob[sl].view(torch.int16) != o1.view(torch.int16)).sum())
                nd = int((db[sl].view(torch.int16) != d1.view(torch.int16)).sum())
                assert nf == 0 and nd == 0, "group %d (budget %d): %d forward / %d dgrad outputs differ" % (gi, budget, nf, nd)
                assert float((sb[gi] - s1[0]).abs().max() / s1[0].abs().max()) < 1e-4
                assert float((bb[gi] - b1[0]).abs().max() / b1[0].abs().max()) < 1e-4


@pytest.mark.parametrize("Cin,H,N,B", FWD_SHAPES)
def test_groups4_weight_gradient_at_full_size(Cin, H, N, B):
    """sv_wgrad with groups = 4 (wgrad3x3w: the groups as an inner loop of every block; wgrad3x3: the groups share the block
    budget) against the sum of four single-group launches, 2e-4 of the gradient's scale."""
    Gn, d = 4, torch.device("cuda:0")
    torch.manual_seed(3 * Cin + H)
    load = _HbmLoad()
    g = G.conv_like(B, H, H, Cin, N, 3, 1, 1)
    ws = torch.empty(16 * 1024 * 1024, device=d)
    x = torch.randn(Gn * B, H, H, Cin, device=d).to(BF)
    dy = (torch.randn(Gn * B, H, H, N, device=d) * 0.05).to(BF)
    sc, sh = (torch.rand(Gn, Cin, device=d) + 0.5).contiguous(), (torch.randn(Gn, Cin, device=d) * 0.3).contiguous()

    def wg(xs, scs, shs, dys, dw, groups):
        L.call("sv_wgrad", C.byref(g), L.SV_BF16, C.c_void_p(xs.data_ptr()), C.c_void_p(scs.data_ptr()),
               C.c_void_p(shs.data_ptr()), 0.01, C.c_void_p(dys.data_ptr()), C.c_void_p(dw.data_ptr()), 0, 1,
               C.c_void_p(ws.data_ptr()), ws.numel(), groups, _st())

    for budget in (512, 256):
        with L.options(persistent_blocks=budget):
            load.kick()
            dwb = torch.zeros(N, 9, Cin, device=d)
            wg(x, sc, sh, dy, dwb, Gn)
            torch.cuda.synchronize()
            dws = torch.zeros(N, 9, Cin, device=d)
            for gi in range(Gn):
                sl = slice(gi * B, (gi + 1) * B)
                wg(x[sl], sc[gi].contiguous(), sh[gi].contiguous(), dy[sl], dws, 1)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(dwb).all())
            err = float((dwb - dws).abs().max() / dws.abs().max())
            assert err < 2e-4, (Cin, H, N, budget, err)


def test_smooth_vae_iteration_at_config5_size():
    """One svhn_VAE smooth-ELBO iteration at BASELINE config 5's per-GPU size, B_u = B_l = 1024, bf16
    (main_smooth_ELBO_svhn.py:228-388): finite, and the loss against the fp32 CPU oracle on the same noise at 2e-2."""
    from oracle import smooth_oracle as SO
    B = 1024
    unl, lab, label, nz = SO.make_inputs("svhn", B, B)
    st = SO.make_state("svhn")
    model = S.SmoothVAE((3, 32, 32), {"cont": 32, "disc": [10]}, temperature=0.67, compute_dtype="bf16").cuda().train()
    model.load_state_dict(st)
    loss_fn = S.SmoothELBOLoss()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    with T.scripted_rng(randn=[nz["eps_u"], nz["eps_l"]], rand=[nz["u_u"], nz["u_l"]]):
        loss = S.smooth_train_step(model, loss_fn, opt, unl.cuda(), lab.cuda(), label.cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    for p in model.parameters():
        assert bool(torch.isfinite(p).all())
    st = {k: v.clone().requires_grad_(True) for k, v in st.items()}
    ref = SO.train_iteration(st, "svhn", unl, lab, label, nz, 1)
    r = float(ref["loss"])
    assert abs(float(loss) - r) <= 2e-2 * abs(r), (float(loss), r)
    # a few more iterations on fresh device noise stay finite and reduce the loss
    last = float(loss)
    for _ in range(5):
        last = float(S.smooth_train_step(model, loss_fn, opt, unl.cuda(), lab.cuda(), label.cuda()))
    assert np.isfinite(last) and last < float(loss)


@pytest.mark.parametrize("workload,names", [
    ("shotvae", ["bn_running_stats", "loss_sup", "loss_unsup", "momentum", "params"]),
    ("svhn", ["adam_m", "adam_v", "loss", "params"])])
def test_bench_plain_run_dumps_the_last_timed_step(tmp_path, workload, names):
    """bench.py without --full: the timed steps only (none of the keys --full adds), `steps` as asked, and --dump-outputs
    writes the last timed step's losses and state -- the losses in the files are the ones in the JSON line.  Two runs with the
    same arguments give that step the same inputs, so their outputs agree to the default mode's rounding (measured at full
    size: relative L2 <= 5e-7, no element off by more than 2e-6 of the array's largest)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for rep in ("a", "b"):
        args = ["--workload", workload, "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / rep)]
        if workload == "svhn":
            args += ["--batch", "64"]
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    out = runs[0]
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    assert not {"roofline", "cpu_baseline", "config4", "wrn28_10_layer_table", "headline_variants", "config5"} & set(out)
    d = tmp_path / "a"
    assert sorted(f[:-4] for f in os.listdir(d)) == names
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    arrays = {n: np.load(d / (n + ".npy")) for n in names}
    for n, x in arrays.items():
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
    assert arrays["params"].size > 1000 and np.abs(arrays["params"]).max() > 0
    if workload == "shotvae":
        assert round(float(arrays["loss_sup"]), 5) == out["loss_sup"]
        assert round(float(arrays["loss_unsup"]), 5) == out["loss_unsup"]
    else:
        assert round(float(arrays["loss"]), 4) == out["loss"]
    for n, x in arrays.items():
        x, y = x.astype(np.float64), np.load(tmp_path / "b" / (n + ".npy")).astype(np.float64)
        scale = max(float(np.abs(x).max()), 1e-30)
        assert float(np.linalg.norm(x - y)) <= 1e-5 * max(float(np.linalg.norm(x)), 1e-30), n
        assert float(np.abs(x - y).max()) <= 1e-4 * scale, n
