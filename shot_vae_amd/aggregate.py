"""The aggregate posterior q(z) = 1/N sum_j q(z | x_j) of a set of encoded images, on the HIP path (csrc/aggpost.hip), and
the diagnostics it gives: the split of the average KL of the SHOT-VAE / smooth-ELBO objectives,

    E_x KL(q(z | x) || p(z)) = I(x; z) + KL(q(z) || p(z)),        KL(q(z) || p(z)) = TC(z) + sum_d KL(q(z_d) || p(z_d)).

    agg = AggregatePosterior(128)
    for image in loader:
        agg.add(*encode_posterior(model, image))
    z, lqx, lpz = agg.sample(mu, ls, key=0, row0=first_row)             # z ~ q(z | x), log q(z | x), log p(z)
    lq, lq_d = agg.log_density(z, per_dim=True)                         # log q(z) [Q], log q(z_d) [Q, D]

    evaluate_aggregate(model, loader)                                   # mi, marginal_kl, total_correlation, dim_kl, ...

`ls` is LOG SIGMA everywhere (encode_posterior halves a smooth model's logvar).  The [queries, gallery, dim] broadcast of the textbook
formulation is never stored; nothing here synchronises with the host, and there is no CPU fallback."""
import math

import torch

from . import _lib as L
from ._latent import _p, _st, eval_only, latent_family, on_device, split_batch
from .neighbors import LatentIndex, posterior_rows

MAX_PARTIALS = 64
TARGET_BLOCKS = 1024          # four blocks per CU of an MI355X: the smallest P that reaches it


def partials(blocks, n):
    """P of a scan whose grid is `blocks` blocks per partial state over a gallery of n rows: enough states to put TARGET_BLOCKS blocks
    on the device, never more than the gallery has tiles of 64 rows, at most 64.  A function of the shapes alone."""
    return max(1, min(MAX_PARTIALS, -(-TARGET_BLOCKS // blocks), -(-n // 64)))


class AggregatePosterior:
    """A device-resident gallery of posteriors (a LatentIndex's doubling buffers) and its mixture density.

    sample() and log_density() issue no host synchronisation and, once the gallery is fixed, can be captured under torch.cuda.graph and
    replayed on new inputs."""

    def __init__(self, dim):
        self.index = LatentIndex(dim, "kl")
        self.dim = self.index.dim

    def __len__(self):
        return len(self.index)

    @property
    def mu(self):
        return self.index.mu[:len(self.index)]

    @property
    def ls(self):
        return self.index.ls[:len(self.index)]

    def add(self, mu, ls):
        """appends the posteriors (mu, ls) [n, dim]; returns the gallery index of the first row added"""
        return self.index.add(mu, ls)

    def sample(self, mu, ls, key=None, row0=0, s=0):
        """-> (z [Q, dim], lqx [Q], lpz [Q]) fp32: z = mu + exp(ls) n(row0 + i, s, .) from the stream of score(samples=S, key=...) -- the
        draw that call uses for image row0 + i and sample s --, log q(z | x) and log p(z).  key: an int or a 1-element int64 device tensor;
        None: z = mu exactly."""
        mu, ls = posterior_rows("AggregatePosterior.sample", L.DIST_KL, mu, ls, dim=self.dim)
        row0, s = int(row0), int(s)
        if row0 < 0 or not 0 <= s < 65536:
            raise ValueError("AggregatePosterior.sample: row0 must be >= 0 and s in [0, 65536)")
        if self.dim > 1 << 18:
            raise ValueError("AggregatePosterior.sample: dim > 2^18 (the generator's counter)")
        if key is not None:
            if torch.is_tensor(key):
                if key.dtype != torch.int64 or key.numel() != 1:
                    raise ValueError("key must be an int or a 1-element int64 device tensor")
                if not key.is_cuda:
                    raise L.ShotVaeHipError("AggregatePosterior.sample: key is not on an MI355X (no CPU fallback)")
                key = key.reshape(1)
            else:
                key = torch.tensor([int(key)], dtype=torch.int64, device=mu.device)
        Q = mu.shape[0]
        z = torch.empty_like(mu)
        lqx = torch.empty(Q, dtype=torch.float32, device=mu.device)
        lpz = torch.empty(Q, dtype=torch.float32, device=mu.device)
        L.call("sv_aggpost_sample", _p(mu), _p(ls), _p(key), row0, s, Q, self.dim, _p(z), _p(lqx), _p(lpz), _st())
        return z, lqx, lpz

    def log_density(self, z, per_dim=False, exclude_self_from=None):
        """-> lq [Q] = log q(z_i) = log 1/N sum_j N(z_i; mu_j, sigma_j^2), fp32; with per_dim also lq_d [Q, dim] = log q(z_id), the
        marginal of every dimension.  exclude_self_from = s: z_i was drawn from gallery row s + i, which is left out of its own sum
        (leave-one-out; the mean is then over N - 1 rows)."""
        on_device("AggregatePosterior.log_density", z)
        if not torch.is_tensor(z) or z.dim() != 2 or z.shape[0] < 1 or z.shape[1] != self.dim:
            raise ValueError("AggregatePosterior.log_density: z must be a non-empty matrix [n, %d]" % self.dim)
        N = len(self.index)
        self_from = -1 if exclude_self_from is None else int(exclude_self_from)
        if self_from < -1:
            raise ValueError("exclude_self_from must be >= 0")
        count = N - 1 if self_from >= 0 else N
        if count < 1:
            raise ValueError("AggregatePosterior.log_density: the gallery is empty" if N == 0 else
                             "AggregatePosterior.log_density: leave-one-out needs two gallery rows")
        z = z.detach().float().contiguous()
        Q, D = z.shape
        passes = [("sv_aggpost_scan", -(-Q // 64), Q)]                    # (entry point, blocks per partial state, outputs)
        if per_dim:
            passes.append(("sv_aggpost_dims", -(-Q // 32) * -(-D // 64), Q * D))
        outs = []
        for name, blocks, R in passes:
            P = partials(blocks, N)
            state = torch.empty(2, P, R, dtype=torch.float64, device=z.device)
            out = torch.empty(R, dtype=torch.float32, device=z.device)
            L.call(name, _p(z), Q, _p(self.index.mu), _p(self.index.ls), N, D, 0, self_from, _p(state[0]), _p(state[1]), P, 1, _st())
            L.call("sv_aggpost_finish", _p(state[0]), _p(state[1]), P, R, count, _p(out), _st())
            outs.append(out)
        return (outs[0], outs[1].view(Q, D)) if per_dim else outs[0]


def _entropy(q):
    return -torch.where(q > 0, q * torch.log(q), torch.zeros_like(q)).sum(dim=-1)


def evaluate_aggregate(model, batches, samples=1, key=0, query_batches=None, per_dim=True):
    """The aggregate-posterior diagnostics of `model` (a VariationalAutoEncoder or a SmoothVAE, in eval mode: NotImplementedError
    otherwise, as for score) over the images of `batches` (image tensors or (image, ...) tuples on the device).  One pass encodes the
    gallery; the queries are the gallery itself, or the images of `query_batches`; query i draws `samples` latents z ~ q(z | x_i) from
    score()'s stream with row0 = its index in the query set, so the estimate does not depend on the batching.  With lqx = log q(z | x),
    lq = log q(z) (the mixture over the gallery), lpz = log p(z), means over queries and samples:

        mi                 mean(lqx - lq)     the mutual information I(x; z) of the image and its latent
        marginal_kl        mean(lq - lpz)     KL(q(z) || p(z)): how far prior samples are from what the decoder was trained on
        kl_c_mc            mean(lqx - lpz)    = mi + marginal_kl by construction: the Monte-Carlo estimate of
        kl_c               the analytic average KL(q(z | x) || p(z)) of the queries
        log_n              log N, the ceiling of `mi`: with the query in the gallery lq >= lqx - log N.  In high dimension the posteriors
                           of different images hardly overlap, the estimate SATURATES there and says nothing beyond "at least log N"
        total_correlation  mean(lq - sum_d lq_d)                                                         (per_dim)
        dim_kl             [D] numpy, KL(q(z_d) || p(z_d)) per dimension: which dimensions are alive     (per_dim)
        dimwise_kl         their sum; marginal_kl = total_correlation + dimwise_kl                       (per_dim)
        active_units       the number of dimensions with Var_x(mu_d) > 0.01 over the gallery (population variance)
        mi_y               the discrete pair: H(mean_i q(y | x_i)) - mean_i H(q(y | x_i)) over the gallery
        marginal_kl_y      log K - H(mean_i q(y | x_i))

    The sums over queries are float64 on the device; the one host read is at the end."""
    from .neighbors import encode_posterior
    family = latent_family("evaluate_aggregate", model)
    samples = int(samples)
    if samples < 1 or samples > 65536:
        raise ValueError("evaluate_aggregate: samples must be in [1, 65536]")
    if key is None:
        raise ValueError("evaluate_aggregate: the samples need a key")
    eval_only("evaluate_aggregate", model)

    def image_of(batch):
        return split_batch("evaluate_aggregate", batch, None)[0]

    def encode_all(image):
        """encode_posterior's (mu, ls) and q(y | x) in float64, from ONE pass of the encoder"""
        if family == "shot":
            mu, ls, la = model.encode(image)
            return mu.float().contiguous(), ls.float().contiguous(), torch.exp(la.double())
        with torch.no_grad():
            mean, logvar, alpha = model.encode(image)
            return mean.float().contiguous(), (0.5 * logvar.float()).contiguous(), alpha.double()

    agg, la_sum, h_sum = None, None, None
    for batch in batches:
        mu, ls, qy = encode_all(image_of(batch))
        if agg is None:
            agg = AggregatePosterior(mu.shape[1])
            la_sum = torch.zeros(qy.shape[1], dtype=torch.float64, device=mu.device)
            h_sum = torch.zeros((), dtype=torch.float64, device=mu.device)
        agg.add(mu, ls)
        la_sum += qy.sum(dim=0)
        h_sum += _entropy(qy).sum()
    if agg is None:
        raise ValueError("evaluate_aggregate: the dataset is empty")
    N, D, dev = len(agg), agg.dim, agg.mu.device
    if not torch.is_tensor(key):
        key = torch.tensor([int(key)], dtype=torch.int64, device=dev)

    if query_batches is None:
        chunk = 8192
        queries = ((agg.mu[a:a + chunk], agg.ls[a:a + chunk]) for a in range(0, N, chunk))
    else:
        queries = (encode_posterior(model, image_of(b)) for b in query_batches)
    acc = torch.zeros(5, dtype=torch.float64, device=dev)         # sums of lqx, lq, lpz, sum_d lq_d, the analytic KL
    dim_acc = torch.zeros(D, dtype=torch.float64, device=dev)     # sums of lq_d - log p(z_d)
    count = 0
    for mu, ls in queries:
        m64, l64 = mu.double(), ls.double()
        acc[4] += 0.5 * (m64 * m64 + torch.exp(2.0 * l64) - 2.0 * l64 - 1.0).sum()
        for s in range(samples):
            z, lqx, lpz = agg.sample(mu, ls, key=key, row0=count, s=s)
            got = agg.log_density(z, per_dim=per_dim)
            lq = got[0] if per_dim else got
            acc[0] += lqx.double().sum()
            acc[1] += lq.double().sum()
            acc[2] += lpz.double().sum()
            if per_dim:
                lqd, z64 = got[1].double(), z.double()
                acc[3] += lqd.sum()
                dim_acc += (lqd + 0.5 * z64 * z64 + 0.5 * math.log(2.0 * math.pi)).sum(dim=0)
        count += mu.shape[0]
    if count == 0:
        raise ValueError("evaluate_aggregate: the query set is empty")
    qbar = la_sum / N
    h_bar = _entropy(qbar)
    var = agg.mu.double().var(dim=0, unbiased=False)
    flat = torch.cat([acc, dim_acc, torch.stack([h_bar, h_sum / N, (var > 0.01).sum().double()])]).cpu().numpy()
    n = float(count * samples)
    lqx, lq, lpz, lqd = (float(flat[i]) / n for i in range(4))
    res = dict(mi=lqx - lq, marginal_kl=lq - lpz, kl_c_mc=lqx - lpz, kl_c=float(flat[4]) / count, log_n=math.log(N),
               active_units=int(flat[5 + D + 2]), mi_y=float(flat[5 + D] - flat[5 + D + 1]),
               marginal_kl_y=math.log(qbar.shape[0]) - float(flat[5 + D]))
    if per_dim:
        res["total_correlation"] = lq - lqd
        res["dim_kl"] = flat[5:5 + D] / n
        res["dimwise_kl"] = float(res["dim_kl"].sum())
    return res
