"""Data parallelism, MI355X-native: one process per GPU, each with a full replica and its shard of the
labelled + unlabelled minibatch; ONE RCCL all-reduce (sum) of the flat fp32 gradient buffer per step
over xGMI, the 1/world scaling folded into the SGD kernel.

Replaces the 11 nn.DataParallel wrappers of the reference (wideresnet.py:78-93, vae.py:108-132,
decoder.py:63-64): no per-forward parameter broadcast, no activation scatter/gather.  Same semantics
where it matters: per-replica BatchNorm statistics, global-batch gradient (equal shards: mean of
per-rank gradients whose losses use the local batch size).  Deviation: mixup / label-smoothing pairs
are drawn inside the shard."""
import os

import torch
import torch.distributed as dist


def init_from_env(backend=None):
    """Initialise torch.distributed from torchrun-style env (RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if (world > 1 or os.environ.get("SV_DP_SINGLE_RANK") == "1") and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"      # "nccl" is RCCL on ROCm
        kw = {}
        if backend == "nccl":
            torch.cuda.set_device(local)
            kw["device_id"] = torch.device("cuda", local)       # the communicator and every barrier on this rank's GPU
        dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)
    return rank, world, local


def active():
    """True when a step must run its collectives: a process group of more than one rank -- or of ONE rank with
    SV_DP_SINGLE_RANK=1, which sends the same RCCL calls (communication stream, async work handles, bucket order) through
    the hardware on a one-GPU box (tests/test_dp_gpu.py; a functional check, the sums are the identity)."""
    return dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("SV_DP_SINGLE_RANK") == "1")


def shard(t, rank, world):
    """Rows [rank*B/world, (rank+1)*B/world) of a batch (SURVEY.md §8e partitioning)."""
    B = t.shape[0]
    if B % world:
        raise ValueError("dp.shard: a batch of %d rows does not divide over %d ranks (the remainder would be dropped silently; "
                         "pad or trim the batch first)" % (B, world))
    per = B // world
    return t[rank * per: (rank + 1) * per]


def broadcast_parameters(model, src=0, optimizer=None):
    """Rank `src`'s parameters, BatchNorm running statistics and num_batches_tracked counters to every rank (start-up).
    After loading a checkpoint on ONE rank also pass the FlatSGD `optimizer`: its momentum buffer and first-step flag are
    broadcast too -- otherwise the ranks would apply different momentum to the same all-reduced gradient and the replicas
    would drift apart from the first step.  Takes the MODEL: the in-place c10d write does not bump any version counter, so
    the engine is told explicitly that its packed weight shadows are stale."""
    if active():
        eng = model._engine
        dist.broadcast(eng.param, src)
        dist.broadcast(eng.bufs, src)
        dist.broadcast(eng.nbt, src)
        eng.mark_dirty()
        if optimizer is not None:
            broadcast_optimizer(optimizer, src)


def broadcast_optimizer(optimizer, src=0):
    """Rank `src`'s FlatSGD state (momentum buffer, number of steps taken, hyper-parameters) to every rank."""
    if not active():
        return
    eng = optimizer.model._engine
    g = optimizer.param_groups[0]
    has_mom = eng.mom is not None and optimizer._steps > 0
    meta = torch.tensor([float(optimizer._steps), 1.0 if has_mom else 0.0, g["lr"], g["momentum"], g["weight_decay"]],
                        dtype=torch.float64, device=eng.param.device)
    dist.broadcast(meta, src)
    steps, has_mom = int(meta[0]), bool(meta[1])
    g["lr"], g["momentum"], g["weight_decay"] = float(meta[2]), float(meta[3]), float(meta[4])
    if has_mom:
        if eng.mom is None or eng.mom.device != eng.param.device:
            eng.mom = torch.zeros_like(eng.param)
        dist.broadcast(eng.mom, src)
        optimizer._steps = steps
    else:
        eng.mom, optimizer._steps = None, 0


def all_reduce_gradients(flat_grad):
    """The single collective of a step.  Returns the scale the optimizer must apply (1/world)."""
    if active():
        _fail_closed(flat_grad)
        dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM)
        return 1.0 / dist.get_world_size()
    return 1.0


def _fail_closed(t):
    """no gradient a failed device-side fork may have corrupted leaves this rank (the sum would spread it to every replica)"""
    if t.is_cuda:
        from . import _lib as L
        L.check_flag_timeouts("before the gradient all-reduce")


class DecoderFirstAllReduce:
    """The step's gradient exchange as TWO buckets, the first overlapped with the encoder's backward (the
    documented fallback to one blocking all-reduce): the decoder's parameters are the tail of the flat buffer and 88 % of
    its bytes (11.3 M of 12.8 M floats for WRN-28-2) and their gradients are complete a third of the way into the backward,
    so their all-reduce is issued on a communication stream as soon as `dgrad:dec0` has been launched; the encoder + heads
    bucket follows after the backward.  Sums over disjoint ranges of one buffer: element for element the same result as
    the single all-reduce (bit-equal at world size 2, tests/test_dp_cpu.py).

        ar = DecoderFirstAllReduce(model)
        ar.arm()                      # before the LAST backward of the step (gradients of earlier backwards accumulate)
        loss.backward()
        scale = ar.finish()           # encoder bucket, wait for both; returns 1 / world for the optimizer

    Without arm() (or when the hook did not fire) finish() is the single all-reduce."""

    def __init__(self, model):
        self.model = model
        self.work = None
        self.comm = None

    def arm(self):
        if active():
            self.work = None
            self.model._engine.bucket_hook = self._decoder_done

    def _decoder_done(self):
        eng = self.model._engine
        tail = eng.grad[eng.plan.dec_off:]
        if tail.is_cuda:
            cur = torch.cuda.current_stream()
            if self.comm is None:
                self.comm = torch.cuda.Stream()
            self.comm.wait_stream(cur)
            side = eng._side.side_of(cur)      # the decoder's weight gradients run there
            if side is not None:
                self.comm.wait_stream(side)
            with torch.cuda.stream(self.comm):
                self.work = dist.all_reduce(tail, op=dist.ReduceOp.SUM, async_op=True)
        else:
            self.work = dist.all_reduce(tail, op=dist.ReduceOp.SUM, async_op=True)

    def finish(self):
        eng = self.model._engine
        eng.bucket_hook = None
        if not active():
            return 1.0
        _fail_closed(eng.grad)
        if self.work is None:
            dist.all_reduce(eng.grad, op=dist.ReduceOp.SUM)
        else:
            dist.all_reduce(eng.grad[:eng.plan.dec_off], op=dist.ReduceOp.SUM)
            self.work.wait()
            if eng.grad.is_cuda and self.comm is not None:
                torch.cuda.current_stream().wait_stream(self.comm)
            self.work = None
        return 1.0 / dist.get_world_size()


def all_reduce_module_gradients(module, average=True):
    """Data parallelism for modules whose parameters are ordinary torch tensors (the smooth-ELBO SmoothVAE, config 5):
    the .grad tensors are flattened into ONE bucket, all-reduced once (RCCL over xGMI) and scattered back, averaged over
    the ranks -- the same single-collective scheme as the flat-buffer path.  Returns the number of elements reduced."""
    grads = [p.grad for p in module.parameters() if p.grad is not None]
    if not grads:
        return 0
    if not active():
        return sum(g.numel() for g in grads)
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    if average:
        flat /= dist.get_world_size()
    off = 0
    for g in grads:
        n = g.numel()
        g.copy_(flat[off:off + n].view_as(g))
        off += n
    return off
