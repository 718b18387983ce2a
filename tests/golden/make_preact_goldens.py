"""Generate the PreActResNet golden vectors by running the REFERENCE implementation on CPU (sibling of make_goldens.py, whose
helpers it uses: the ``.cuda()`` no-op shim, the scripted host RNG, the driver of the step of main_shot_vae.py:280-366).

Runs only where the reference checkout is mounted (make_goldens.REF, read-only).  Weights, inputs and noise are the closed forms of
oracle/closed_form.py over the PreActResNet key table of tests/_preact_oracle.py -- check_key_table() below holds that table to the
reference's own state_dict (keys, order, shapes) before any fixture is written -- so the fixtures hold the reference's OUTPUTS only.

    python tests/golden/make_preact_goldens.py

Writes tests/golden/ref_state_keys_preact.json, ref_step_preact18_br.npz, ref_eval_preact18.npz, ref_eval_preact34.npz.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import torch                                  # noqa: E402
import make_goldens as MG                     # noqa: E402
from tests import _preact_oracle as P         # noqa: E402


def run_keys_case(tag):
    """state_dict keys + shapes of the reference model, in its order, for both data_parallel layouts"""
    VAE, *_ = MG.import_reference()
    rec = {}
    for name in ("preactresnet18", "preactresnet34"):
        for dp in (False, True):
            model = VAE(encoder_name=name, num_input_channels=3, drop_rate=0, img_size=(32, 32), data_parallel=dp,
                        continuous_latent_dim=128, disc_latent_dim=10, sample_temperature=0.67, small_input=True)
            rec["%s|K=10|dp=%d" % (name, int(dp))] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    with open(os.path.join(HERE, tag + ".json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    print(tag, {k: len(v) for k, v in rec.items()})
    return rec


def check_key_table(rec):
    """the closed-form state (oracle.closed_form.make_state over tests/_preact_oracle.state_shapes) has the reference's keys, in its
    order, with its shapes"""
    from oracle import closed_form as C
    for name in ("preactresnet18", "preactresnet34"):
        with P.patched():
            st = C.make_state(name, K=10)
        ref = rec["%s|K=10|dp=0" % name]
        assert list(st.keys()) == [k for k, _ in ref], name
        assert all(list(st[k].shape) == shape for k, shape in ref), name


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), "reference not mounted; goldens are generated in the build container"
    torch.set_num_threads(8)
    check_key_table(run_keys_case("ref_state_keys_preact"))
    with P.patched():          # oracle.closed_form.make_state over the PreActResNet key table
        MG.run_eval_case("ref_eval_preact18", "preactresnet18", 10, 4)
        MG.run_eval_case("ref_eval_preact34", "preactresnet34", 10, 4)
        # B = 8: the smallest batch whose 4 x 4 maps fill one 128-pixel tile of the stride-1 3x3 kernels (eight whole images)
        MG.run_step_case("ref_step_preact18_br", "preactresnet18", 10, 8, 8, True)
