"""gather_codes on a real MI355X, for both model families: regrouped to chunk_rows the gathered rows do not depend on how the caller
batched the images, and taken as they come they are encode_posterior's rows of every batch, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import shot_vae_amd as S                                        # noqa: E402
from shot_vae_amd import _latent as LT                          # noqa: E402
from tests import _knn_ref as KR                                # noqa: E402

N = 12


@pytest.mark.parametrize("kind", KR.EVAL_KINDS)
def test_gather_codes_regroups_and_gathers_bit_for_bit(kind):
    from tests.test_cluster_gpu import eval_model
    model = eval_model(kind)                                    # wideresnet-10-1 / the smooth model of test_cluster_cpu: 32x32, fp32, eval
    images = KR.eval_images(kind)[2][:N].to("cuda:0")
    labels = ((torch.arange(N) * 3 + 1) % KR.EVAL_CLASSES).to("cuda:0")
    split = [(images[:5], labels[:5]), (images[5:], labels[5:])]
    whole = [(images, labels)]

    a = LT.gather_codes("test", model, split, chunk_rows=4)
    b = LT.gather_codes("test", model, whole, chunk_rows=4)
    assert all(tuple(t.shape)[0] == N for t in a) and a[2].dtype == torch.int64
    for got, want in zip(a, b):
        assert torch.equal(got, want)
    assert torch.equal(a[2], labels)

    x, ls, y = LT.gather_codes("test", model, split, chunk_rows=None)
    parts = [S.encode_posterior(model, image) for image, _ in split]
    assert torch.equal(x, torch.cat([p[0] for p in parts])) and torch.equal(ls, torch.cat([p[1] for p in parts])) and torch.equal(y, labels)
