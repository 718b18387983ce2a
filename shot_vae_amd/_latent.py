"""What the latent-space analysis modules (neighbors, aggregate, quality, cluster, calibration, embed, mixture, probe, propagate) share
on the host side: launch helpers, input checks, the model gate, batch handling, label budgets and the grid-residency rule (DESIGN.md
4n).  The kernels stay with their modules.  A check that needs no device comes first: shape, then the calling module's own limits, then
the no-CPU rule.  Model classes and encode_posterior are imported inside the functions that need them: nothing here imports a sibling
at module level."""
import ctypes as C

import torch

from . import _lib as L

COMPUTE_UNITS, LDS_PER_CU = 256, 160 * 1024          # an MI355X


# ---- launch helpers ----
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- input checks ----
def on_device(what, *tensors):
    """the no-CPU rule: a tensor among `tensors` that is on the host is refused (anything that is no tensor is skipped)"""
    for t in tensors:
        if torch.is_tensor(t) and not t.is_cuda:
            raise L.ShotVaeHipError("%s: input is not on an MI355X (no CPU fallback)" % what)


def matrix(what, x, dim=None, owner="the model", limit=None):
    """x as a contiguous fp32 device matrix [n, d] of `owner`'s `dim` columns.  The shape checks come first (they need no device), then
    limit(n) -- the caller's own check of its sizes against the number of rows --, then the no-CPU rule"""
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s: x must be a non-empty matrix [n, d]" % what)
    if dim is not None and x.shape[1] != dim:
        raise ValueError("%s: x has %d columns, %s %d" % (what, x.shape[1], owner, dim))
    if limit is not None:
        limit(x.shape[0])
    on_device(what, x)
    return x.detach().float().contiguous()


def labels(what, y, n):
    """y as a contiguous int64 device vector [n]"""
    if not torch.is_tensor(y) or y.dim() != 1 or y.shape[0] != n or y.dtype.is_floating_point or y.dtype == torch.bool:
        raise ValueError("%s: y must be an integer vector [%d]" % (what, n))
    if not y.is_cuda:
        raise L.ShotVaeHipError("%s: labels are not on an MI355X (no CPU fallback)" % what)
    return y.detach().long().contiguous()


def vectors(what, *tensors):
    """non-empty vectors of one length (a None among them is skipped); the shape checks come first, then the no-CPU rule"""
    n = None
    for t in tensors:
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dim() != 1 or t.numel() < 1 or (n is not None and t.numel() != n):
            raise ValueError("%s: non-empty vectors%s" % (what, "" if n is None else " of one length [%d]" % n))
        n = t.numel()
    on_device(what, *tensors)
    return [None if t is None else t.detach() for t in tensors]


# ---- the model gate: three functions, because every evaluate_* checks its own arguments between the first and the second ----
def latent_family(what, model):
    """-> "shot" (a VariationalAutoEncoder) or "smooth" (a SmoothVAE); anything else is a TypeError"""
    from .smooth import SmoothVAE
    from .vae import VariationalAutoEncoder
    if isinstance(model, VariationalAutoEncoder):
        return "shot"
    if isinstance(model, SmoothVAE):
        return "smooth"
    raise TypeError("%s: a VariationalAutoEncoder or a SmoothVAE, not %s" % (what, type(model).__name__))


def eval_only(what, model):
    if model.training:
        raise NotImplementedError("%s is implemented for eval mode only (no noise, no gradients): call model.eval() first" % what)


def num_classes(model):
    """the width of the discrete code, without an encoder pass"""
    return model._plan.K if latent_family("num_classes", model) == "shot" else model.latent_disc_dim


# ---- batches ----
def _pair(what, batch):
    if not isinstance(batch, (tuple, list)) or len(batch) < 2:
        raise ValueError("%s: the batches must be (image, label) tuples" % what)
    on_device(what, batch[0], batch[1])
    return batch[0], batch[1]


def split_batch(what, batch, need_label):
    """-> (image, label or None) of one batch, on the device.  need_label True: an (image, label) tuple or a ValueError; False: an
    image tensor, (image,) or (image, label); None: whatever follows the image is not read.  A label comes back as an int64 vector
    with one entry per image."""
    if need_label:
        image, label = _pair(what, batch)
    else:
        image, label = (batch[0], batch[1] if len(batch) > 1 else None) if isinstance(batch, (tuple, list)) else (batch, None)
        if need_label is None:
            label = None
        on_device(what, image, label)
    if label is not None:
        label = label.reshape(-1).long()
        if label.numel() != image.shape[0]:
            raise ValueError("%s: %d labels for %d images" % (what, label.numel(), image.shape[0]))
    return image, label


def regroup(what, batches, rows):
    """the (image, label) batches as they come (rows = None), or regrouped into batches of exactly `rows` rows (the last one smaller)"""
    held, n = [], 0
    for batch in batches:
        image, label = _pair(what, batch)
        if rows is None:
            yield image, label
            continue
        held.append((image, label.reshape(-1)))
        n += image.shape[0]
        while n >= rows:
            image, label = (torch.cat([h[i] for h in held]) if len(held) > 1 else held[0][i] for i in (0, 1))
            yield image[:rows], label[:rows]
            held, n = ([(image[rows:], label[rows:])] if n > rows else []), n - rows
    if n:
        yield tuple(torch.cat([h[i] for h in held]) if len(held) > 1 else held[0][i] for i in (0, 1))


def gather_codes(what, model, batches, space="mu", chunk_rows=None, need_label=True):
    """-> (x [n, d], ls [n, d] or None, labels int64 [n] or None), the rows of all batches in order: encode_posterior's (mu, log sigma)
    (space "mu"), or model.features() and ls = None (space "features").  chunk_rows: the (image, label) batches are regrouped to that
    many rows before the model sees them (the encoders' last bits depend on the batch size); None takes them as they come.  Without
    need_label the labels are None as soon as one batch carries none."""
    from .neighbors import encode_posterior
    xs, lss, ys, labelled = [], [], [], True
    for batch in batches if chunk_rows is None else regroup(what, batches, int(chunk_rows)):
        image, label = split_batch(what, batch, need_label)
        x, ls = encode_posterior(model, image) if space == "mu" else (model.features(image).float().contiguous(), None)
        xs.append(x)
        lss.append(ls)
        if label is None:
            labelled = False
        else:
            ys.append(label)
    if not xs:
        raise ValueError("%s: the dataset is empty" % what)
    return torch.cat(xs), (torch.cat(lss) if space == "mu" else None), (torch.cat(ys) if labelled else None)


# ---- budgets and arguments ----
def label_budgets(what, labels_per_class):
    """None (all labels), a budget m or a list of budgets (None among them: all) -> the list, validated"""
    budgets = list(labels_per_class) if isinstance(labels_per_class, (list, tuple)) else [labels_per_class]
    for m in budgets:
        if m is not None and (isinstance(m, bool) or int(m) != m or int(m) < 1):
            raise ValueError("%s: a budget must be None or an integer >= 1, not %r" % (what, m))
    if len(set(budgets)) != len(budgets):
        raise ValueError("%s: a budget is listed twice" % what)
    return budgets


def take_args(args, names):
    """pops those of `names` that `args` holds -> a dict of them (what goes to fit() out of an evaluator's **args)"""
    return {name: args.pop(name) for name in names if name in args}


# ---- the grid-residency rule ----
def resident_partials(p, blocks, per_cu):
    """P of an accumulation whose blocks walk their rows one after the other: aggregate.partials' p, lowered until the grid of
    p x `blocks` blocks is resident at once with `per_cu` blocks on a compute unit -- a second round of blocks would double the time --,
    never below 1.  A function of the shapes alone: P fixes the summation order."""
    return max(1, min(p, COMPUTE_UNITS * per_cu // blocks))
