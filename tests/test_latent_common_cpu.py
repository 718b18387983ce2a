"""The host layer the latent-space analysis modules share (shot_vae_amd._latent), without a GPU: regrouping, the order of the input
checks, the label budgets and the grid-residency rule against the three kernels' own grid descriptions.  Where the logic under test
runs behind the no-CPU rule, the tensors are host tensors of a subclass that says it is on the device: nothing here launches."""
import pytest
import torch

from shot_vae_amd import _latent as LT
from shot_vae_amd import _lib as L
from shot_vae_amd import aggregate as AG
from shot_vae_amd import cluster as CL
from shot_vae_amd import mixture as MX
from shot_vae_amd import probe as PB


class OnDevice(torch.Tensor):
    is_cuda = property(lambda self: True)


def dev(t):
    return t.as_subclass(OnDevice)


def batches_of(sizes):
    """(image [n, 2], label [n]) batches whose rows are numbered through: image row r is [r, r], its label r"""
    out, at = [], 0
    for n in sizes:
        rows = torch.arange(at, at + n)
        out.append((dev(torch.stack([rows, rows], dim=1).float()), dev(rows.clone())))
        at += n
    return out


# ================================================================================================ batches
@pytest.mark.parametrize("sizes,want", [((5, 7), [4, 4, 4]), ((5, 6), [4, 4, 3]), ((12,), [4, 4, 4]), ((1, 1, 1), [3]), ((4, 4), [4, 4])])
def test_regroup_cuts_the_rows_into_chunks_in_order(sizes, want):
    got = list(LT.regroup("t", batches_of(sizes), 4))
    assert [int(image.shape[0]) for image, _ in got] == want == [int(label.shape[0]) for _, label in got]
    image, label = torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])
    assert torch.equal(label, torch.arange(sum(sizes))) and torch.equal(image[:, 0], label.float())


def test_regroup_without_rows_hands_the_batches_through():
    batches = batches_of((5, 7))
    got = list(LT.regroup("t", batches, None))
    assert len(got) == 2 and all(g[0] is b[0] and g[1] is b[1] for g, b in zip(got, batches))
    assert list(LT.regroup("t", [], 4)) == []


def test_regroup_and_split_batch_refuse_what_is_no_pair_or_not_on_the_device():
    x, y = torch.zeros(5, 2), torch.zeros(5, dtype=torch.int64)
    for rows in (None, 4):
        with pytest.raises(ValueError, match=r"\(image, label\)"):
            list(LT.regroup("t", [dev(x)], rows))
        with pytest.raises(L.ShotVaeHipError, match="t: input is not on an MI355X"):
            list(LT.regroup("t", [(x, y)], rows))
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            list(LT.regroup("t", [(dev(x), y)], rows))
    for batch in (dev(x), (dev(x),)):
        with pytest.raises(ValueError, match=r"\(image, label\)"):
            LT.split_batch("t", batch, True)
        image, label = LT.split_batch("t", batch, False)
        assert image is (batch[0] if isinstance(batch, tuple) else batch) and label is None
    for need in (True, False):
        with pytest.raises(L.ShotVaeHipError, match="MI355X"):
            LT.split_batch("t", (dev(x), y), need)
        with pytest.raises(ValueError, match="4 labels for 5 images"):
            LT.split_batch("t", (dev(x), dev(y[:4])), need)
        image, label = LT.split_batch("t", (dev(x), dev(y.int().reshape(5, 1))), need)
        assert label.dtype == torch.int64 and tuple(label.shape) == (5,)
    assert LT.split_batch("t", (dev(x), y[:4], "more"), None)[1] is None           # what follows the image is not read
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        LT.split_batch("t", x, None)


# ================================================================================================ input checks
def test_matrix_checks_the_shape_then_the_callers_limit_then_the_device():
    x = torch.zeros(6, 8)

    def limit(n):
        raise ValueError("t: more than %d rows asked for" % n)

    for bad in (x.view(-1), torch.zeros(0, 8), torch.zeros(6, 0), None):
        with pytest.raises(ValueError, match="non-empty matrix"):
            LT.matrix("t", bad, limit=limit)
    with pytest.raises(ValueError, match="x has 8 columns, the probe 5"):
        LT.matrix("t", x, 5, "the probe", limit)
    with pytest.raises(ValueError, match="more than 6 rows"):
        LT.matrix("t", x, 8, "the probe", limit)
    with pytest.raises(L.ShotVaeHipError, match="t: input is not on an MI355X"):
        LT.matrix("t", x, 8, "the probe", lambda n: None)
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        LT.matrix("t", x)
    got = LT.matrix("t", dev(x.double()), 8)
    assert got.dtype == torch.float32 and got.is_contiguous()


def test_labels_and_vectors_check_the_shape_before_the_device():
    y = torch.zeros(6, dtype=torch.int64)
    for bad in (y[:5], y.float(), y.bool(), y.view(2, 3), None):
        with pytest.raises(ValueError, match=r"integer vector \[6\]"):
            LT.labels("t", bad, 6)
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        LT.labels("t", y, 6)
    assert LT.labels("t", dev(y.int()), 6).dtype == torch.int64
    for bad in ((y, y[:5]), (y.view(2, 3),), (y[:0],)):
        with pytest.raises(ValueError, match="non-empty vectors"):
            LT.vectors("t", *bad)
    with pytest.raises(L.ShotVaeHipError, match="MI355X"):
        LT.vectors("t", dev(y), None, y)
    assert LT.vectors("t", dev(y), None)[1] is None


# ================================================================================================ budgets and arguments
def test_label_budgets_accepts_none_a_number_or_a_list():
    assert LT.label_budgets("t", None) == [None]
    assert LT.label_budgets("t", 5) == [5]
    assert LT.label_budgets("t", [10, None, 100]) == [10, None, 100]
    assert LT.label_budgets("t", (3,)) == [3]
    for bad in (True, 0, 2.5, [4, -1]):
        with pytest.raises(ValueError, match="t: a budget must be None or an integer >= 1"):
            LT.label_budgets("t", bad)
    with pytest.raises(ValueError, match="t: a budget is listed twice"):
        LT.label_budgets("t", [5, 5])


def test_take_args_pops_what_it_names():
    args = dict(tol=None, seed=3, max_iter=7)
    assert LT.take_args(args, ("max_iter", "tol", "check_every")) == dict(max_iter=7, tol=None) and args == dict(seed=3)


# ================================================================================================ the residency rule
def lowered(p, blocks, resident):
    """the rule as the three modules first wrote it: P goes down one at a time until the grid fits"""
    while p > 1 and p * blocks > resident:
        p -= 1
    return p


def test_resident_partials_is_the_rule_of_the_three_accumulation_kernels():
    for k in (1, 3, 16, 17, 64, 65, 257, 513, 1024):
        for dim in (1, 5, 32, 33, 128, 1000):
            tiles = (1 if k <= 16 else -(-k // 64)) * -(-dim // 32)                  # sv_gmm_accum's and sv_probe_accum's grid
            blocks = -(-dim // CL._slice(k)) + 1                                     # sv_kmeans_accum's
            per_cu = max(1, min(4, 160 * 1024 // (k * CL._slice(k) * 8)))
            for n in (1, 64, 65, 100, 4096, 50000):
                for mod in (MX, PB):
                    p = mod._partials(k, dim, n)
                    assert 1 <= p <= 64 and p <= -(-n // 64) and (p == 1 or p * tiles <= 512), (mod.__name__, k, dim, n)
                    assert p == lowered(AG.partials(tiles, n), tiles, 512) == LT.resident_partials(AG.partials(tiles, n), tiles, 2)
                p = CL._partials(k, dim, n)
                assert 1 <= p <= 64 and p <= -(-n // 64) and (p == 1 or p * blocks <= 256 * per_cu), (k, dim, n)
                assert p == lowered(AG.partials(blocks * 4 // per_cu, n), blocks, 256 * per_cu)
    assert LT.resident_partials(64, 1000, 2) == 1 and LT.resident_partials(64, 8, 2) == 64 and LT.resident_partials(64, 9, 2) == 56
    assert (LT.COMPUTE_UNITS, LT.LDS_PER_CU) == (256, 160 * 1024)
