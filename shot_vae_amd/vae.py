"""Drop-in for the reference's ``shot_vae_model.vae.VariationalAutoEncoder`` (vae.py:89-151) whose
forward/backward run as hand-written HIP kernels on MI355X.

Same constructor, same positional ``forward`` signature, same 4-tuple result, same ``state_dict``
keys (with or without the ``.module`` segments ``data_parallel=True`` produces in the reference), so
the loop of main_shot_vae.py:261-383 runs unchanged.  Differences (all documented in DESIGN.md):
  * ``data_parallel`` only selects the key naming; multi-GPU is one process per GPU + one RCCL
    all-reduce of the flat gradient buffer (see dp.py), not nn.DataParallel;
  * gradients of the parameters are accumulated by the kernels straight into one flat fp32 buffer
    (``p.grad`` are views of it);
  * the wideresnet-D-W and preactresnet18 / preactresnet34 encoders on 32x32 inputs are implemented;
  * dropout (``drop_rate``) draws one int64 key per training forward (torch.randint, in front of that forward's
    noise) and regenerates its masks from it in the kernels (shotvae_hip.h, sv_dropout_args): the masks differ from
    torch's nn.Dropout draws, their distribution does not;
  * in eval mode the halves of the forward are calls of their own (extension): encode / features / predict, decode, reconstruct,
    generate, and the sub-modules feature_extractor(x) / feature_reconstructor(latent) are callable with the reference's shapes
    and meaning (vae.py:142,150); the other sub-modules only carry parameters.
"""
import collections
import math
import weakref

import torch
from torch import nn

from . import _lib as L
from .engine import Engine, Plan, encoder_family


# model.score(): the per-image terms of the ELBO, fp32 [B] each; elbo = -(recon + kl_c + kl_d)
Scores = collections.namedtuple("Scores", ["recon", "kl_c", "kl_d", "elbo"])


class _Node(nn.Module):
    """Name-space module: only carries parameters / buffers so state_dict keys match the reference."""

    def forward(self, *a, **k):
        raise RuntimeError("this sub-module is a parameter container; call the VariationalAutoEncoder")


class _EntryNode(_Node):
    """A name-space module that is also callable like the reference's sub-module of that name: the call goes to the method `entry`
    of the owning model (FlatModule.ENTRY_NODES), looked up when it is called.  The owner is held weakly -- a child that referred to
    its parent strongly would make a cycle, and the model with its flat device buffers would be freed by the cycle collector only."""

    def __init__(self, owner, entry):
        super(_EntryNode, self).__init__()
        self._owner, self._entry = weakref.ref(owner), entry

    def forward(self, *a, **k):
        owner = self._owner()
        if owner is None:
            raise RuntimeError("this sub-module outlived the model it belongs to")
        return getattr(owner, self._entry)(*a, **k)


def _dp_key(key, wrapped):
    """the data_parallel=True spelling of `key`; wrapped = Plan.dp_wrapped, the modules the reference wraps in nn.DataParallel
    (wideresnet.py:78-93, preactresnet.py:94-112, vae.py:108-132, decoder.py:63-64)"""
    for w in wrapped:
        if key.startswith(w + "."):
            return w + ".module." + key[len(w) + 1:]
    return key


class _VAEFunction(torch.autograd.Function):
    """One autograd node for the whole network (one or several batched instances of it): fused HIP forward,
    hand-written HIP backward."""

    @staticmethod
    def forward(ctx, anchor, model, image, groups, eps, u, rec_groups=None, update_order=None, keys=None):
        eng = model._engine
        rec, mu, ls, la, f = eng.forward(image, groups, eps, u, model._temperature, model.training, keep=True,
                                         rec_groups=rec_groups, update_order=update_order, keys=keys)
        ctx.model, ctx.f = model, f
        # an output that enters no loss term arrives as None in backward (not as a zero tensor): the reconstruction of
        # the mixed forwards (main_shot_vae.py:311,356) -- their decoder backward is then skipped, as autograd does in the
        # reference
        ctx.set_materialize_grads(False)
        return rec, mu, ls, la

    @staticmethod
    def backward(ctx, d_rec, d_mu, d_ls, d_la):
        model, f = ctx.model, ctx.f
        if f is None:
            raise RuntimeError("backward through the same SHOT-VAE forward twice is not supported")
        if not f.training:
            # an eval-mode forward normalises with the running statistics and saves no batch statistics: the
            # batch-statistics BatchNorm backward below would read uninitialised mean / rstd
            raise NotImplementedError("backward through an eval-mode forward (BatchNorm with running statistics) is not "
                                      "implemented; the reference never does it (main_shot_vae.py:423-424: no_grad)")
        ctx.f = None
        model._attach_grads()
        eng = model._engine
        eng.backward(f, d_rec.contiguous().float() if d_rec is not None else None, d_mu, d_ls, d_la)
        return (None,) * 9


def check_drop_rate(drop_rate):
    """nn.Dropout's range check, and the one rate the kernels do not take"""
    drop_rate = float(drop_rate)
    if math.isnan(drop_rate) or drop_rate < 0 or drop_rate > 1:
        raise ValueError("dropout probability has to be between 0 and 1, but got {}".format(drop_rate))
    if drop_rate == 1:
        raise NotImplementedError("drop_rate == 1 is not supported: the whole tensor into norm2 would be zero, and its "
                                  "BatchNorm has no batch statistics to normalise with")
    return drop_rate


class FlatModule(nn.Module):
    """A network whose parameters, gradients and BatchNorm buffers live in an Engine's flat buffers: the module tree only names
    views of them, under the reference's state_dict keys (either data_parallel layout).  Shared by VariationalAutoEncoder and
    WideResNetClassifier (classifier.py)."""

    TOP_MODULES = ()          # the reference's top-level sub-modules, in its registration order
    ENTRY_NODES = {}          # top-level sub-module -> name of the method a call of it runs (the others only carry parameters)

    def _init_flat(self, plan, compute_dtype, data_parallel, rng, drop_rate):
        self._plan = plan
        self._engine = Engine(plan, compute_dtype)
        self._data_parallel = data_parallel
        self.rng = rng
        self.drop_rate = drop_rate
        # debugging aid: the int64 [G] dropout-key tensor of every training forward with drop_rate > 0, in call order (the
        # step functions clear it when they start; at most the last 16 are kept).  With these, a test regenerates each
        # forward's masks (sv_dropout_mask).
        self.last_dropout_keys = []
        self._views = []          # (parameter, flat offset/spec) for re-pointing after device moves
        self._anchor = None
        # in-place updates by a torch optimizer bump the parameters' version counters: that is how the
        # engine learns that its packed weight shadows are stale
        self._engine.version_probe = lambda: sum(v[0]._version for v in self._views)

    # ------------------------------------------------------------------ module tree / state_dict
    def _node(self, path):
        m = self
        for part in path:
            if not hasattr(m, part):
                m.add_module(part, _Node())
            m = getattr(m, part)
        return m

    def _flat_view(self, flat, kind, payload):
        if kind == "conv":
            return payload.torch_view(flat)
        if kind == "mat":
            off, (r, c) = payload
            return flat[off: off + r * c].view(r, c)
        off, n = payload
        return flat[off: off + n]

    def _build_tree(self):
        eng, plan = self._engine, self._plan
        for name in self.TOP_MODULES:
            self.add_module(name, _EntryNode(self, self.ENTRY_NODES[name]) if name in self.ENTRY_NODES else _Node())
        for key, kind, payload in plan.state_items():
            k = _dp_key(key, plan.dp_wrapped) if self._data_parallel else key
            parts = k.split(".")
            node = self._node(parts[:-1])
            if kind in ("conv", "mat", "vec"):
                prm = nn.Parameter(self._flat_view(eng.param, kind, payload))
                node.register_parameter(parts[-1], prm)
                self._views.append((prm, kind, payload))
            elif kind == "rm":
                node.register_buffer(parts[-1], eng.bufs[payload.rm_off: payload.rm_off + payload.C])
            elif kind == "rv":
                node.register_buffer(parts[-1], eng.bufs[payload.rv_off: payload.rv_off + payload.C])
            else:
                node.register_buffer(parts[-1], eng.nbt[payload.index])

    def _repoint(self):
        """Make every Parameter / buffer a view of the (possibly moved) flat storage again."""
        eng, plan = self._engine, self._plan
        for prm, kind, payload in self._views:
            prm.data = self._flat_view(eng.param, kind, payload)
            prm.grad = None
        for key, kind, payload in plan.state_items():
            if kind in ("rm", "rv", "nbt"):
                k = _dp_key(key, plan.dp_wrapped) if self._data_parallel else key
                parts = k.split(".")
                node = self._node(parts[:-1])
                if kind == "rm":
                    t = eng.bufs[payload.rm_off: payload.rm_off + payload.C]
                elif kind == "rv":
                    t = eng.bufs[payload.rv_off: payload.rv_off + payload.C]
                else:
                    t = eng.nbt[payload.index]
                node._buffers[parts[-1]] = t

    def _apply(self, fn, recurse=True):
        # keep ONE flat storage: move the flat buffers, then re-point the views (nn.Module._apply would
        # give every parameter its own allocation)
        self._engine.to(fn)
        self._repoint()
        self._anchor = None
        return self

    def _attach_grads(self):
        """p.grad = view of the flat gradient buffer.  If the optimizer dropped them
        (zero_grad(set_to_none=True)), the flat buffer is zeroed first."""
        eng = self._engine
        first = self._views[0][0]
        if first.grad is not None and first.grad.data_ptr() == eng.grad.data_ptr() + 4 * self._views[0][2].master_off:
            return
        eng.grad.zero_()
        for prm, kind, payload in self._views:
            prm.grad = self._flat_view(eng.grad, kind, payload)

    def load_state_dict(self, state_dict, strict=True):
        """Accepts both the data_parallel=True ('.module.') and =False key layouts of the reference."""
        own = set(self.state_dict().keys())
        fixed = {}
        for k, v in state_dict.items():
            if k in own:
                fixed[k] = v
                continue
            plain = k.replace(".module.", ".")
            alt = _dp_key(plain, self._plan.dp_wrapped) if self._data_parallel else plain
            fixed[alt if alt in own else k] = v
        out = super(FlatModule, self).load_state_dict(fixed, strict)
        self._engine.mark_dirty()
        return out

    # ------------------------------------------------------------------ flat buffers, dropout keys
    def flat_parameters(self):
        """(param, grad) flat fp32 buffers: what FlatSGD updates and dp.all_reduce reduces."""
        return self._engine.param, self._engine.grad

    def _drop_active(self):
        return self.training and self.drop_rate > 0

    def _draw_keys(self, n, dev):
        """n dropout keys (int64, on dev): host RNG -> the CPU generator and a copy, device RNG -> the device generator.
        torch.randint, never randn / rand: those carry the sampler's noise."""
        if self.rng == "host":
            return torch.randint(0, 2 ** 63 - 1, (n,), dtype=torch.int64).to(dev)
        return torch.randint(0, 2 ** 63 - 1, (n,), dtype=torch.int64, device=dev)

    def _log_keys(self, keys):
        self.last_dropout_keys.append(keys)
        del self.last_dropout_keys[:-16]


class VariationalAutoEncoder(FlatModule):
    TOP_MODULES = ("feature_extractor", "global_avg", "continuous_inference", "disc_latent_inference", "sample", "feature_reconstructor")
    # callable with the reference's shapes and meaning (vae.py:142,150), in eval mode
    ENTRY_NODES = {"feature_extractor": "_feature_extractor", "feature_reconstructor": "_feature_reconstructor"}

    def __init__(self, encoder_name, num_input_channels=1, drop_rate=0, img_size=(160, 160), data_parallel=True,
                 continuous_latent_dim=100, disc_latent_dim=10, sample_temperature=0.67, small_input=False,
                 compute_dtype="bf16", rng="host"):
        super(VariationalAutoEncoder, self).__init__()
        # wideresnet-D-W, preactresnet18 / 34; densenet and the bottleneck PreActResNets exist in the reference (vae.py:93-104) but
        # are not built: NotImplementedError, the reference's fall-through error type (vae.py:106); an unknown preactresnet* name
        # is the reference's KeyError (preactresnet.py:131)
        encoder_family(encoder_name)
        drop_rate = check_drop_rate(drop_rate)
        if not small_input:
            raise NotImplementedError("small_input=False (7x7 stem + max-pool) is not implemented; the "
                                      "CIFAR/SVHN configs of main_shot_vae.py use small_input=True")
        if tuple(img_size) != (32, 32):
            raise NotImplementedError("only 32x32 inputs are implemented")
        plan = Plan(encoder_name, in_ch=num_input_channels, img=img_size[0], ldc=continuous_latent_dim,
                    K=int(disc_latent_dim), drop_rate=drop_rate)
        self._init_flat(plan, compute_dtype, data_parallel, rng, drop_rate)
        self._temperature = sample_temperature
        self._disc_latent_dim = disc_latent_dim
        self._engine.init_default()
        self._build_tree()
        self.feature_extractor.num_feature_channel = plan.cfeat

    # ------------------------------------------------------------------ reference API
    def _draw_noise(self, B, dev, gumbel):
        """noise in the reference's order: randn for z (vae.py:37,82), then rand for gumbel (vae.py:52,69).  With dropout in
        training mode the forward's key comes first (the encoder runs before the sampler, vae.py:140-151): (eps, u, key)"""
        plan = self._plan
        key = self._draw_keys(1, dev) if self._drop_active() else None
        if self.rng == "host":
            eps = torch.randn(B, plan.ldc).to(dev)
            u = torch.rand(B, plan.K).to(dev) if gumbel else None
        else:
            eps = torch.randn(B, plan.ldc, device=dev)
            u = torch.rand(B, plan.K, device=dev) if gumbel else None
        return eps, u, key

    @staticmethod
    def _group_spec(mixup, disc_label, disc_pseudo_label, mixup_lam):
        """(mode, label, label_mix, lam) of one forward call's arguments (vae.py:38-52)"""
        if disc_label is None:
            return (0, None, None, 0.0)
        label = disc_label.view(-1).long().contiguous()
        if mixup:
            lam = mixup_lam.reshape(1).float() if torch.is_tensor(mixup_lam) else float(mixup_lam)
            return (2, label, disc_pseudo_label.view(-1).long().contiguous(), lam)
        return (1, label, None, 0.0)

    def forward(self, input_img, mixup=False, disc_label=None, disc_pseudo_label=None, mixup_lam=None):
        if not input_img.is_cuda:
            raise L.ShotVaeHipError("VariationalAutoEncoder: input is not on an MI355X (no CPU fallback)")
        spec = self._group_spec(mixup, disc_label, disc_pseudo_label, mixup_lam)
        eps, u, key = self._draw_noise(input_img.size(0), input_img.device, spec[0] == 0)
        return self._run(input_img, [spec], eps, u, keys=key)

    def forward_groups(self, images, specs, eps=None, u=None, rec_groups=None, update_order=None, keys=None):
        """Several forward calls as ONE batched launch sequence (extension; see Engine.forward): images = list of equally
        sized batches, specs = list of dicts with the keyword arguments of forward() (mixup, disc_label,
        disc_pseudo_label, mixup_lam).  Equivalent to calling forward() on each batch -- every group keeps its own
        BatchNorm batch statistics and the running statistics receive the groups' momentum updates in list order -- at a
        fraction of the launches.  eps / u: the noise to use ([G * B, ldc] / [G * B, K]); drawn here if None, group by
        group in the reference's order.  rec_groups = Gd: only the first Gd batches' reconstructions are produced and
        differentiated (the others' last ConvTranspose and decoder backward are skipped; reconstruction is [Gd * B, ...]);
        update_order[k] = the list position of the reference's k-th forward (order of the BatchNorm running-statistic
        updates; default list order).  keys: the dropout keys (int64 [G] on the device; drop_rate > 0 in training mode only),
        drawn here if None.  Returns the 4-tuple of forward() with the groups concatenated along dim 0."""
        G = len(images)
        B = images[0].size(0)
        if any(im.size(0) != B for im in images):
            raise ValueError("forward_groups: the batches must have equal sizes")
        dev = images[0].device
        gs = [self._group_spec(sp.get("mixup", False), sp.get("disc_label"), sp.get("disc_pseudo_label"),
                               sp.get("mixup_lam")) for sp in specs]
        if eps is None:
            pairs = [self._draw_noise(B, dev, g[0] == 0) for g in gs]
            eps = torch.cat([e for e, _, _ in pairs])
            if any(uu is not None for _, uu, _ in pairs):
                z = torch.zeros(B, self._plan.K, device=dev)
                u = torch.cat([uu if uu is not None else z for _, uu, _ in pairs])
            if keys is None and self._drop_active():
                keys = torch.cat([k for _, _, k in pairs])
        if keys is None and self._drop_active():
            keys = self._draw_keys(G, dev)
        return self._run(torch.cat([im.float() for im in images]), gs, eps, u, rec_groups, update_order, keys)

    def forward_groups_direct(self, images, specs, eps, u, rec_groups=None, update_order=None, image_cat=None, x16=None,
                              keys=None, want_rec=True):
        """forward_groups for a caller that runs the backward itself (no autograd node): returns (rec, mu, ls, la, ctx); pass
        ctx and the gradients w.r.t. the four outputs to backward_direct().  image_cat / x16: the concatenated images and
        their NHWC16 form when the caller has already made them (train_step_grouped's input-side stream); with x16 alone the
        images are not concatenated (and `images` is not read).  keys: the dropout keys (int64 [G] on the device), required in
        training mode with drop_rate > 0.  want_rec=False: rec is None, the logits stay in ctx.h[5] (Engine.forward)."""
        gs = [self._group_spec(sp.get("mixup", False), sp.get("disc_label"), sp.get("disc_pseudo_label"),
                               sp.get("mixup_lam")) for sp in specs]
        with torch.no_grad():
            if image_cat is None and x16 is None:
                image_cat = torch.cat([im.float() for im in images])
            if self._drop_active():
                self._log_keys(keys)
            return self._engine.forward(image_cat, gs, eps, u, self._temperature, self.training, keep=True,
                                        rec_groups=rec_groups, update_order=update_order, x16=x16,
                                        keys=keys if self._drop_active() else None, want_rec=want_rec)

    def backward_direct(self, ctx, d_rec, d_mu, d_ls, d_la, own_grads=False, d_rec_nhwc=False):
        """accumulates the parameter gradients of a forward_groups_direct() call into the flat gradient buffer (p.grad).
        own_grads: d_mu / d_ls / d_la are the caller's own, freshly written tensors and may be modified in place;
        d_rec_nhwc: d_rec is the NHWC gradient of the decoder's last layer (Engine.backward)"""
        if not ctx.training:
            raise NotImplementedError("backward through an eval-mode forward (BatchNorm with running statistics) is not implemented")
        self._attach_grads()
        with torch.no_grad():
            self._engine.backward(ctx, d_rec, d_mu, d_ls, d_la, own_grads, d_rec_nhwc)

    # ------------------------------------------------------------------ inference API (eval mode only; extension)
    # The halves of the eval-mode forward as calls of their own (Engine.encode / latent_draw / decode).  BatchNorm normalises with
    # the running statistics; nothing here updates them or touches the gradients, and no output requires grad.

    def _infer_check(self, what, *tensors):
        if self.training:
            raise NotImplementedError("%s is implemented for eval mode only (BatchNorm with the running statistics, no "
                                      "gradients): call model.eval() first" % what)
        for t in tensors:
            if torch.is_tensor(t) and not t.is_cuda:
                raise L.ShotVaeHipError("VariationalAutoEncoder.%s: input is not on an MI355X (no CPU fallback)" % what)

    def _key_tensor(self, key):
        """a generator key as sv_latent_draw reads it: a 1-element int64 device tensor (an int is copied to the device)"""
        if torch.is_tensor(key):
            if key.dtype != torch.int64 or key.numel() != 1:
                raise ValueError("key must be an int or a 1-element int64 device tensor")
            return key.reshape(1)
        return torch.tensor([int(key)], dtype=torch.int64, device=self._engine.param.device)

    def _class_args(self, c, B):
        """latent_draw's class arguments of `c`: an int64 label vector [B] or a float class matrix [B, K]"""
        if c.dtype == torch.int64 and c.dim() == 1 and c.size(0) == B:
            return dict(label=c.contiguous())
        if c.is_floating_point() and tuple(c.shape) == (B, self._plan.K):
            return dict(cls=c.float().contiguous())
        raise ValueError("the class argument must be an int64 label vector [%d] or a float class matrix [%d, %d]"
                         % (B, B, self._plan.K))

    def encode(self, image):
        """(mu [B, ldc], log_sigma [B, ldc], log_alpha [B, K]) of `image`: the encoder and the inference heads only -- what the
        eval model(image) returns behind its reconstruction, without the sampler, the decoder and the reconstruction's copy."""
        self._infer_check("encode", image)
        with torch.no_grad():
            return self._engine.encode(image)

    def features(self, image):
        """the pooled encoder features [B, C] (the input of the inference heads, vae.py:143)"""
        self._infer_check("features", image)
        with torch.no_grad():
            return self._engine.encode(image, want_feat=True)[3]

    def predict(self, image):
        """the predicted class, int64 [B]: argmax of log_alpha, on the device (no host synchronisation)"""
        self._infer_check("predict", image)
        with torch.no_grad():
            return self._engine.encode(image)[2].argmax(dim=1)

    def decode(self, z, c, sigmoid=False):
        """The decoder's output [B, ch, 32, 32] (raw logits, or their sigmoid) for the continuous latent z [B, ldc] and the class c:
        an int64 label vector [B] (one-hot; a label outside [0, K) selects no class) or a float class matrix [B, K]."""
        return self._decode("decode", z, c, sigmoid)

    def _decode(self, what, z, c, sigmoid):
        self._infer_check(what, z, c)
        if z.dim() != 2 or z.size(1) != self._plan.ldc:
            raise ValueError("%s: z must be [B, %d]" % (what, self._plan.ldc))
        with torch.no_grad():
            eng = self._engine
            latent = eng.latent_draw(z.size(0), mu=z.float().contiguous(), **self._class_args(c, z.size(0)))
            return eng.decode(latent, "sigmoid" if sigmoid else "logits")

    def reconstruct(self, image, label=None, sample=False, key=None):
        """sigmoid of the reconstruction of `image` from its posterior mean (sample=True: from a posterior sample drawn with `key`,
        an int or a 1-element int64 device tensor; None: one torch.randint draw, as for a dropout key -- it advances torch's generator) under its predicted class -- or under `label`
        (int64 [B]): the class-swap "analogy"."""
        self._infer_check("reconstruct", image, label)
        with torch.no_grad():
            eng = self._engine
            mu, ls, la = eng.encode(image)
            if sample:
                key = self._draw_keys(1, image.device) if key is None else self._key_tensor(key)
            cls = dict(label=label.view(-1).long().contiguous()) if label is not None else dict(cls=la, argmax=True)
            latent = eng.latent_draw(mu.size(0), mu=mu, ls=ls if sample else None, key=key if sample else None, **cls)
            return eng.decode(latent, "sigmoid")

    def generate(self, labels, key, tau=1.0, row0=0, dtype="float"):
        """Class-conditional samples: z ~ N(0, tau^2 I) from the counter-based stream of sv_latent_draw (a sample depends only on
        key, row0 + its row and the column: a batch drawn in one call equals the same rows drawn in several), c = one-hot(labels)
        (int64 [B] on the device).  key: an int, or a 1-element int64 device tensor (read on the device: a captured call is
        replayed with another key by writing it there).  dtype "float": sigmoid images [B, ch, 32, 32] fp32; "uint8": pixels
        [B, 32, 32, ch] uint8, the layout DeviceDataset takes."""
        self._infer_check("generate", labels, key)
        if dtype not in ("float", "uint8"):
            raise ValueError("generate: dtype must be 'float' or 'uint8'")
        with torch.no_grad():
            eng = self._engine
            labels = labels.view(-1).long().contiguous()
            latent = eng.latent_draw(labels.size(0), key=self._key_tensor(key), tau=tau, row0=row0, label=labels)
            return eng.decode(latent, "sigmoid" if dtype == "float" else "uint8")

    def _score_args(self, what, image, criterion, label, samples, key):
        """the checks score() and log_likelihood() share -> (label, key) as the engine takes them.  Mode first, then the arguments'
        values, then where the tensors live: a wrong argument is reported as such on any machine."""
        self._infer_check(what)
        p = self._plan
        if image.dim() != 4 or tuple(image.shape[1:]) != (p.in_ch, p.img, p.img):
            raise ValueError("%s: the images must be [B, %d, %d, %d]" % (what, p.in_ch, p.img, p.img))
        samples = int(samples)
        if samples < 1 or samples > 65536:
            raise ValueError("%s: samples must be in [1, 65536]" % what)
        if getattr(criterion, "discrete_dim", p.K) != p.K:
            raise ValueError("%s: the criterion is built for %d classes, the model for %d" % (what, criterion.discrete_dim, p.K))
        if not criterion.bce_reconstruction and not float(criterion.x_sigma) > 0:
            raise ValueError("%s: x_sigma must be > 0" % what)
        if key is None:
            if samples != 1:
                raise ValueError("%s: key=None scores at z = mu, which is one sample; samples=%d needs a key" % (what, samples))
        elif (key.dtype != torch.int64 or key.numel() != 1) if torch.is_tensor(key) else (isinstance(key, bool) or not isinstance(key, int)):
            raise ValueError("%s: key must be an int or a 1-element int64 device tensor" % what)
        if label is not None and (not torch.is_tensor(label) or label.dtype != torch.int64 or label.numel() != image.size(0)):
            raise ValueError("%s: label must be an int64 vector [%d]" % (what, image.size(0)))
        self._infer_check(what, image, label, key)
        return (label.reshape(-1).contiguous() if label is not None else None), (self._key_tensor(key) if key is not None else None)

    def score_terms(self, image, criterion, want, label=None, samples=1, key=None, row0=0, normalised=True, chunk_rows=None,
                    what="score_terms"):
        """The outputs named in `want` -- any of "recon", "kl_c", "kl_d", "elbo", "log_px" -- of one pass over `image`, as a dict of
        fp32 [B] device tensors: what score() and log_likelihood() are made of, for a caller that wants both from the same draws
        (evaluate_scores).  Arguments as for those two; `what` names the call in error messages."""
        row0 = int(row0)
        if row0 < 0:
            raise ValueError("%s: row0 must be >= 0" % what)
        label, key = self._score_args(what, image, criterion, label, samples, key)
        add = 0.0
        if "log_px" in want and normalised and not criterion.bce_reconstruction:
            # the normalising constant of the Gaussian likelihood (the Bernoulli likelihood of BCE mode has none)
            p = self._plan
            add = -0.5 * p.in_ch * p.img * p.img * math.log(2.0 * math.pi * float(criterion.x_sigma) ** 2)
        with torch.no_grad():
            return self._engine.score(image, criterion.bce_reconstruction, criterion.x_sigma, label, samples, key, row0, want=tuple(want),
                                      log_px_add=add, chunk_rows=chunk_rows)

    def score(self, image, criterion, label=None, samples=1, key=None, row0=0):
        """Scores(recon, kl_c, kl_d, elbo) of every image, fp32 [B] on the device: the reconstruction term of
        `criterion` (its bce_reconstruction and x_sigma) averaged over `samples` draws z ~ q(z | x) from the counter-based stream of
        sv_latent_sweep (key: an int, or a 1-element int64 device tensor, as for generate; an image's draws depend only on key, row0 +
        its row, the sample and the column) -- or at z = mu exactly with key=None (samples == 1) -- and over the classes: the exact
        expectation under q(y | x) with label=None, the class label[b] (int64 [B]) otherwise; the two KL terms in closed form."""
        out = self.score_terms(image, criterion, Scores._fields, label, samples, key, row0, what="score")
        return Scores(*[out[w] for w in Scores._fields])

    def log_likelihood(self, image, criterion, samples, key, label=None, row0=0, normalised=True, chunk_rows=None):
        """The importance-weighted bound on log p(x) of every image (log p(x | y = label) with labels), fp32 [B] on the device:
        log 1/S sum_s p(x | z_s) p(z_s) / q(z_s | x), z_s ~ q(z | x) from the stream of score(), p(x | z) = 1/K sum_k p(x | z, k)
        (label=None) -- a lower bound in expectation that tightens with `samples`.  The decoder runs over B * S * K rows (B * S with
        labels) in chunks of at most chunk_rows (default Engine.SCORE_CHUNK_ROWS = 8192: under 1 GB of eval scratch on
        wideresnet-28-2 in bf16, under 2 GB in fp32).  normalised: MSE mode includes the Gaussian's -(D / 2) log(2 pi x_sigma^2)."""
        if key is None:
            raise ValueError("log_likelihood: a key is required (an int or a 1-element int64 device tensor)")
        return self.score_terms(image, criterion, ("log_px",), label, samples, key, row0, normalised, chunk_rows,
                                what="log_likelihood")["log_px"]

    def _feature_extractor(self, x):
        """model.feature_extractor(x): the encoder's output map [B, C, h, h] (behind the transition BatchNorm + activation)"""
        self._infer_check("feature_extractor", x)
        with torch.no_grad():
            return self._engine.encoder_map(x)

    def _feature_reconstructor(self, latent):
        """model.feature_reconstructor(latent [B, ldc + K, 1, 1]): the decoder's raw logits"""
        self._infer_check("feature_reconstructor", latent)
        p = self._plan
        if latent.dim() != 4 or tuple(latent.shape[1:]) != (p.ldc + p.K, 1, 1):
            raise ValueError("feature_reconstructor: the latent must be [B, %d, 1, 1]" % (p.ldc + p.K))
        flat = latent.reshape(latent.size(0), p.ldc + p.K).float()
        return self._decode("feature_reconstructor", flat[:, :p.ldc].contiguous(), flat[:, p.ldc:].contiguous(), False)

    def _run(self, image, groups, eps, u, rec_groups=None, update_order=None, keys=None):
        eng = self._engine
        dev = image.device
        if not self._drop_active():
            keys = None
        elif keys is not None:
            self._log_keys(keys)
        if torch.is_grad_enabled():
            if self._anchor is None or self._anchor.device != dev:
                self._anchor = torch.zeros(1, device=dev, requires_grad=True)
            return _VAEFunction.apply(self._anchor, self, image, groups, eps, u, rec_groups, update_order, keys)
        rec, mu, ls, la, _ = eng.forward(image, groups, eps, u, self._temperature, self.training, keep=False,
                                         rec_groups=rec_groups, update_order=update_order, keys=keys)
        return rec, mu, ls, la
