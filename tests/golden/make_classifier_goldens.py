"""Generate the classifier-baseline golden vectors by running the REFERENCE implementation on CPU (sibling of
make_preact_goldens.py; it uses make_goldens.py's ``.cuda()`` no-op shim and sample indices).

Runs only where the reference checkout is mounted (make_goldens.REF, read-only).  Weights and inputs are the closed forms of
oracle/closed_form.py over the classifier key table of tests/_classifier_oracle.py -- check_key_table() holds that table to the
reference's own state_dict (keys, order, shapes) before any fixture is written -- so the fixtures hold the reference's OUTPUTS only.
Beside every reference run the oracle runs in fp64: a recorded quantity at which the reference's own fp32 result is further than
1e-5 (relative) from fp64 stops the script -- choose another batch for that case, do not loosen a gate.

    python tests/golden/make_classifier_goldens.py

Writes tests/golden/ref_cls_state_keys.json, ref_cls_step_wrn10_1.npz, ref_cls_step_wrn28_2.npz, ref_cls_step_wrn28_10_k100.npz,
ref_cls_eval_wrn10_1.npz.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np                            # noqa: E402
import torch                                  # noqa: E402
import make_goldens as MG                     # noqa: E402
from tests import _classifier_oracle as Q     # noqa: E402

FP64_BOUND = 1e-5


def import_reference():
    MG.import_reference()                     # the .cuda() shim and the reference on sys.path
    from classifier_model.wideresnet import get_wide_resnet
    return get_wide_resnet


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def run_keys_case(tag):
    """state_dict keys + shapes of the reference model, in its order, for both data_parallel layouts"""
    get_wide_resnet = import_reference()
    rec = {}
    for name, K in Q.KEY_CASES:
        for dp in (False, True):
            model = get_wide_resnet(name, 0, input_channels=3, num_classes=K, small_input=True, data_parallel=dp)
            rec["%s|K=%d|dp=%d" % (name, K, int(dp))] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(HERE, tag + ".json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    print(tag, {k: len(v) for k, v in rec.items()})
    return rec


def check_key_table(rec):
    """the closed-form state over tests/_classifier_oracle.state_shapes has the reference's keys, in its order, with its shapes"""
    for name, K in Q.KEY_CASES:
        st = Q.make_state(name, K)
        ref = rec["%s|K=%d|dp=0" % (name, K)]
        assert list(st.keys()) == [k for k, _ in ref], name
        assert all(list(st[k].shape) == shape for k, shape in ref), name


def reference_model(name, K):
    get_wide_resnet = import_reference()
    model = get_wide_resnet(name, 0, input_channels=3, num_classes=K, small_input=True, data_parallel=False)
    st = Q.make_state(name, K)
    assert list(model.state_dict().keys()) == list(st.keys()), "state_dict key order mismatch"
    model.load_state_dict(st)
    return model


def run_step_case(tag):
    name, K, B, steps, stream0 = Q.STEP_CASES[tag]
    model = reference_model(name, K)
    model.train()
    criterion = torch.nn.CrossEntropyLoss()
    opt = torch.optim.SGD(model.parameters(), **Q.SGD)
    opt.zero_grad()
    names = [k for k, _ in model.named_parameters()]
    rec = {}
    for s in range(steps):                    # main_classifier.py:191-198
        image, label = Q.make_batch(B, K, s, stream0=stream0)
        logits = model(image)
        loss = criterion(logits, label)
        loss.backward()
        rec["s%d.logits" % s] = logits.detach().numpy().copy()
        rec["s%d.loss" % s] = np.array(float(loss.detach()))
        if s == 0:
            rec["s0.grad_norm"] = np.array([float(p.grad.double().norm()) for _, p in model.named_parameters()])
            rec["s0.grad_sample"] = np.concatenate([p.grad.reshape(-1)[torch.from_numpy(MG.grad_sample_idx(p.numel()))].numpy()
                                                    for _, p in model.named_parameters()])
        opt.step()
        opt.zero_grad()
    sd = model.state_dict()
    rec["final.param_norm"] = np.array([float(sd[k].double().norm()) for k in names])
    rec["final.param_sample"] = np.concatenate([sd[k].reshape(-1)[torch.from_numpy(MG.grad_sample_idx(sd[k].numel()))].numpy()
                                                for k in names])
    for k, v in sd.items():
        if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
            rec["final.buf." + k] = v.numpy()
    rec["meta.param_names"] = np.array(names)
    # the reference's own fp32 error, against the oracle in fp64
    outs, st, pk = Q.run_steps(name, K, B, steps, stream0, dt=torch.float64)
    assert pk == names
    err = {}
    for s in range(steps):
        err["s%d.logits" % s] = rel(rec["s%d.logits" % s], outs[s]["logits"].numpy())
        err["s%d.loss" % s] = abs(float(rec["s%d.loss" % s]) - float(outs[s]["loss"])) / max(1.0, abs(float(outs[s]["loss"])))
    err["s0.grad_norm"] = float(np.max(np.abs(rec["s0.grad_norm"] - outs[0]["grad_norm"]) / outs[0]["grad_norm"].max()))
    err["s0.grad_sample"] = rel(rec["s0.grad_sample"], outs[0]["grad_sample"])
    pn = np.array([float(st[k].detach().norm()) for k in pk])
    err["final.param_norm"] = float(np.max(np.abs(rec["final.param_norm"] - pn) / pn))
    ps = np.concatenate([st[k].detach().reshape(-1)[torch.from_numpy(Q.sample_idx(st[k].numel()))].numpy() for k in pk])
    err["final.param_sample"] = rel(rec["final.param_sample"], ps)
    err["final.buf"] = max(rel(v, st[k[len("final.buf."):]].numpy()) for k, v in rec.items() if k.startswith("final.buf."))
    print(tag, "fp32 reference against the fp64 oracle:", {k: "%.2e" % v for k, v in err.items()})
    bad = {k: v for k, v in err.items() if not v <= FP64_BOUND}
    assert not bad, "the reference's fp32 run is further than %g from fp64 at %s: choose another batch" % (FP64_BOUND, bad)
    np.savez_compressed(os.path.join(HERE, tag + ".npz"), **rec)
    print(tag, "loss", [float(rec["s%d.loss" % s]) for s in range(steps)], "bytes", os.path.getsize(os.path.join(HERE, tag + ".npz")))


def run_eval_case():
    tag, name, K, B = Q.EVAL_CASE
    model = reference_model(name, K)
    model.eval()
    image, label = Q.make_batch(B, K, 0)
    with torch.no_grad():                     # main_classifier.py:222-237
        logits = model(image)
        loss = torch.nn.CrossEntropyLoss()(logits, label)
        score = torch.softmax(logits, dim=1)
    _, y_pred = torch.topk(score, k=5, dim=1)
    y_true = label.view(-1, 1)
    rec = dict(logits=logits.numpy(), loss=np.array(float(loss)), top1=np.array(int(torch.sum(y_true == y_pred[:, :1]))),
               top5=np.array(int(torch.sum(y_true == y_pred))))
    o = Q.run_eval(name, K, B, dt=torch.float64)
    err = dict(logits=rel(rec["logits"], o["logits"].numpy()), loss=abs(float(loss) - float(o["loss"])) / max(1.0, abs(float(o["loss"]))))
    print(tag, "fp32 reference against the fp64 oracle:", {k: "%.2e" % v for k, v in err.items()}, "top1 / top5", int(rec["top1"]), int(rec["top5"]))
    assert all(v <= FP64_BOUND for v in err.values()), err
    assert (o["top1"], o["top5"]) == (int(rec["top1"]), int(rec["top5"]))
    np.savez_compressed(os.path.join(HERE, tag + ".npz"), **rec)


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), "reference not mounted; goldens are generated in the build container"
    torch.set_num_threads(8)
    check_key_table(run_keys_case("ref_cls_state_keys"))
    for tag in Q.STEP_CASES:
        run_step_case(tag)
    run_eval_case()
