"""Conditional GAN (pix2pix-style) on the same HIP kernels as the CVAE.

The reference documents this model (trained_models/README.md:95-144, the pickled generator
structure, ``GAN_Painter(...).paint(input, z, transform, inverse_transform)`` at
scripts/create_lightcone.py:47-54) but its code lives in an un-vendored external module, so there
is nothing to be bit-compatible with: parity is **unpinned**  and is checked against
this repository's own torch restatement (oracle/cgan_torch.py) only.

What is fixed by the reference's tables and what is a choice made here:
  * generator / discriminator layer tables, LeakyReLU(0.2), spectral norm on every discriminator
    layer, Adam(lr 5e-5, betas (0.5, 0.999)), lr x0.85 every 1568 iterations, batch 6, lambda 2.5,
    redshift conditioning f(z) = z - 1 as a constant input plane            -- from the reference;
  * losses: BCE on the discriminator's sigmoid output (README's loss levels D~ln2, G_adv~ln2/2 fit
    0.5*(BCE(real,1)+BCE(fake,0)) and 0.5*BCE(fake,1)); the "perceptual" term is NOT defined in the
    reference -- an L1 distance between generated and true field is used            -- chosen here.
"""
import ctypes as C
import os

import torch

from .. import _lib as L
from .arch import cgan_discriminator_architecture, cgan_generator_architecture
from .graph import PlanBase, SNConv2d, Slot, build_holders, compile_sequential, _stream
from . import paint_graph as PG


class _GanPlan(PlanBase):
    """The training plan: generator, discriminator (both halves, and the fake half alone) and their backward passes.

    ``train_dtype="bf16"``: the residual blocks of the generator, and only they, run on the bf16 matrix-core kernels with
    bf16 slots -- both convolutions of every block (forward, data gradient, weight gradient), the block tails forward and
    backward, the batch-norm and activation backward passes between them.  The k9 stem, both stride-2 encoders, both
    transposed decoders, the k9 head, the whole discriminator, the losses, spectral norm and the optimizer (fp32 master
    weights) read and write fp32.  The biased 64 <-> 128 boundary layers stay fp32 on purpose (unlike the paint plan): the
    bf16 training epilogues take no bias and there is no bf16 weight gradient for their shapes.  Two ``CastUnit`` s stand at
    the ends of the trunk.  A tensor is rounded to bf16 (to nearest even) at exactly these points:

      forward
        * entry: A0 = leaky(batchnorm(raw)) of the last encoder, from its fp32 raw output and batch statistics, rounded
          once and stored -- the operand of the first block's first convolution AND that block's skip;
        * the weights of the residual convolutions (the packed images; the master weights and dW stay fp32);
        * the stored raw output of every residual convolution (fp32 accumulation, one rounding; its batch statistics are
          those of the values as stored);
        * the staged activated input of every residual convolution, leaky(batchnorm(stored raw)), in the forward and again,
          from the same values, in the weight gradient (a block's first convolution reads a stored block output: no-op);
        * every block's output, leaky(batchnorm(raw) + skip);
        * exit: the last block's stored output is converted exactly to fp32 for the decoder.
      backward (every gradient tensor of a bf16 slot is bf16)
        * exit: the decoder's fp32 data gradient, rounded once;
        * g_t of a block tail, (d1 + d2) * leaky'(out), the sum of the block output's consumers formed in fp32;
        * d(loss)/d(raw) of both convolutions of a block (the batch-norm backward map, evaluated in fp32);
        * the data gradient of both convolutions (fp32 accumulation, one rounding);
        * entry: d1 + d2 of A0's two consumers (first convolution, skip), summed in fp32, rounded once, then converted
          exactly to fp32; the encoder's fp32 activation and batch-norm backward follows unchanged.

    The weight gradients accumulate in fp32 and are reduced in a fixed order: two iterations from one state are bit-equal."""

    TRAIN_DTYPES = ("fp32", "bf16")

    def __init__(self, model, n):
        self.model, self.lib, self.device, self.impl, self.sync = model, model._lib, model.device, L.IMPL_AUTO, model.sync
        self.n, self.ws = n, None
        self.train_dtype = getattr(model, "train_dtype", "fp32")
        if self.train_dtype not in self.TRAIN_DTYPES:
            raise ValueError(f"train_dtype {self.train_dtype!r}: one of {self.TRAIN_DTYPES}")
        self._bf16_convs, self._bf16_first, self._f32_first = \
            self.bf16_policy(model.g_arch) if self.train_dtype == "bf16" else ((), None, None)
        H, W = model.tile_size, model.tile_size
        dev = self.device
        self.y2 = Slot.new(n, H, W, 2, dev)
        gu, gs, tr = compile_sequential(self, "generator.", model.g_arch, model.generator, self.y2,
                                        need_input_grad=False)
        if [t[0] for t in tr] != ["tanh"]:
            raise NotImplementedError("the generator must end in conv + tanh")
        if gs.shape() != (n, H, W, 1) or gs.pw is not None:
            raise ValueError(f"generator output {gs.shape()}")
        self.g_units, self.g_raw = gu, gs
        for u in self.flat_units(gu):
            if self.bf16_unit(u.name) != bool(u.bf16):      # (a missing kernel is an error, never a quiet fp32 layer)
                raise NotImplementedError(f"{u.name}: the bf16 training kernels do not take this layer")
        # discriminator input: [dm, z-1, pressure] for the real (first n) and the fake (last n) half
        self.d_in = Slot.new(2 * n, H, W, 3, dev, cstride=4)
        # (the discriminator step needs no d(loss)/d(input): its first layer computes no data gradient)
        du, ds, tr = compile_sequential(self, "discriminator.", model.d_arch, model.discriminator, self.d_in,
                                        need_input_grad=False)
        if [t[0] for t in tr] != ["sigmoid"]:
            raise NotImplementedError("the discriminator must end in conv + sigmoid")
        self.d_units, self.d_raw = du, ds
        if ds.c != 1 or ds.pw is not None:
            raise ValueError("discriminator head must be a single raw channel")
        # The generator step goes through the discriminator for d(loss)/d(fake) only.  The discriminator has no batch-norm,
        # so D(fake) does not depend on the real half and the real half's gradients are exactly zero: a second set of units
        # over the FAKE half alone (same parameter holders, n images instead of 2n) does half the work of the full pass,
        # and its first layer's data gradient is restricted to the generated channel.
        self.d_in_fake = Slot(self.d_in.buf[n:], n, H, W, 3, 0)
        du2, ds2, _ = compile_sequential(self, "discriminator.", model.d_arch, model.discriminator, self.d_in_fake,
                                         need_input_grad=True)
        du2[0].restrict_dgrad(2, 3)
        self.d_units_fake, self.d_raw_fake = du2, ds2
        self.x_nchw = torch.zeros((n, 1, H, W), device=dev)
        self.sums = torch.zeros(4, device=dev, dtype=torch.float64)
        self.need_ws(256 * 8)
        for u in reversed(du):
            u.prepare_backward()
        for u in reversed(du2):
            u.prepare_backward()
        for u in reversed(gu):
            u.prepare_backward()
        self.ws = torch.zeros(max(self.ws_bytes, 256) // 8 + 32, device=dev, dtype=torch.float64)
        self.ws_bytes = self.ws.numel() * 8
        # weight gradients on a second stream beside the data-gradient chain (graph.ConvUnit.conv_backward)
        self.side = None
        if os.environ.get("BP_SIDE_WGRAD", "1") != "0":
            self.side = torch.cuda.Stream(device=dev)
            self.ws2 = torch.zeros_like(self.ws)
        n_, h_, w_ = self.d_in.n, H, W
        di = self.d_in
        self.v_real_cond = L.View(di.buf.data_ptr(), n, h_, w_, 2, di.cstride, 0)
        self.v_fake_cond = L.View(di.buf[n:].data_ptr(), n, h_, w_, 2, di.cstride, 0)
        self.v_real_x = L.View(di.buf.data_ptr(), n, h_, w_, 1, di.cstride, 2)
        self.v_fake_x = L.View(di.buf[n:].data_ptr(), n, h_, w_, 1, di.cstride, 2)
        self.v_real = L.View(di.buf.data_ptr(), n, h_, w_, 3, di.cstride, 0)        # [dm, aux, pressure] of the real half
        self.d_in_fake.ensure_grad()
        self.v_dfake = L.View(self.d_in_fake.grad_buf.data_ptr(), n, h_, w_, 1, di.cstride, 2)
        self.cnt_d = float(n * ds.h * ds.w)           # discriminator outputs per half
        self.cnt_px = float(n * H * W)

    # ---- bf16 policy of ``train_dtype="bf16"`` (see the class docstring)
    @staticmethod
    def bf16_policy(g_arch, prefix="generator."):
        """(name prefixes of the convolutions that run and store bf16: the bodies of the residual blocks; name of the first
        block: it reads bf16; name of the convolution behind the last block: it reads fp32).  Needs no device."""
        names = [layer[0].lower() for layer in g_arch]
        res = [i for i, nm in enumerate(names) if nm == "residual block"]
        if not res:
            return (), None, None
        convs = [i for i, nm in enumerate(names) if nm in ("conv", "transp conv")]
        if res != list(range(res[0], res[-1] + 1)) or not any(i < res[0] for i in convs) \
                or not any(i > res[-1] for i in convs):
            raise NotImplementedError("train_dtype='bf16': the residual blocks must stand together between two convolutions")
        return (tuple(f"{prefix}{i}.res_block." for i in res), f"{prefix}{res[0]}",
                f"{prefix}{min(i for i in convs if i > res[-1])}")

    def bf16_unit(self, name):
        return name.startswith(self._bf16_convs) if self._bf16_convs else False

    bf16_out = bf16_unit

    def in_dtype(self, name):
        return L.BF16 if name == self._bf16_first else L.F32 if name == self._f32_first else None

    # ---- forward pieces
    def generate(self, y, zc, training):
        lib, st = self.lib, _stream()
        self._keep = (y.contiguous(), zc.reshape(self.n, 1).contiguous())
        L.check(lib.bp_nchw_to_view(L.ptr(self._keep[0]), 1, L.ptr(self._keep[1]), 1, C.byref(self.y2.view), st),
                "generator input")
        self.forward_g(training)

    def forward_g(self, training):
        """The generator over ``y2`` as it stands; fake = tanh(g_raw), written into the pressure channel of the fake half
        of the D input."""
        for u in self.g_units:
            u.forward(training)
        L.check(self.lib.bp_unary_forward(C.byref(self.g_raw.view), None, 1, C.byref(self.v_fake_x), _stream()), "tanh")

    def fill(self, fn):
        """Let ``fn`` write the step's inputs in place of ``generate``'s and ``load_real``'s copies:
        ``fn(gen_in, d_real, d_fake_cond, x_nchw)`` receives the generator's input ``y2.view`` (c = 2: [dm, aux]), the real
        half of ``d_in`` as one view (c = 3: [dm, aux, pressure]), the conditioning channels of the fake half (c = 2) and
        the dense ``x_nchw`` tensor (pressure).  It owns exactly those channels: the pad channel of ``d_in`` belongs to
        ``Slot.new`` and the fake half's pressure channel to the generator's tanh.  ``fn`` enqueues on the current stream."""
        fn(self.y2.view, self.v_real, self.v_fake_cond, self.x_nchw)

    def load_real(self, x):
        lib, st = self.lib, _stream()
        self.x_nchw.copy_(x)
        y, zc = self._keep
        for v in (self.v_real_cond, self.v_fake_cond):
            L.check(lib.bp_nchw_to_view(L.ptr(y), 1, L.ptr(zc), 1, C.byref(v), st), "condition planes")
        L.check(lib.bp_nchw_to_view(L.ptr(self.x_nchw), 1, None, 0, C.byref(self.v_real_x), st), "real field")

    def discriminate(self, training, fake_only=False):
        for h in self.model.sn_layers:
            h.refresh(training)
        for u in (self.d_units_fake if fake_only else self.d_units):
            u.forward(training)

    def d_losses(self):
        """sums[0] = sum BCE(real, 1), sums[1] = sum BCE(fake, 0), sums[2] = sum BCE(fake, 1)."""
        lib, st, n, r = self.lib, _stream(), self.n, self.d_raw
        for k, (n0, n1, t) in enumerate(((0, n, 1.0), (n, 2 * n, 0.0), (n, 2 * n, 1.0))):
            L.check(lib.bp_bce_logits(C.byref(r.view), n0, n1, t, L.ptr(self.sums[k:]), L.ptr(self.ws), self.ws_bytes,
                                      st), "bce")

    def g_adv_loss(self):
        """sums[2] = sum BCE(D(fake), 1) from the fake-half units (generator step)."""
        L.check(self.lib.bp_bce_logits(C.byref(self.d_raw_fake.view), 0, self.n, 1.0, L.ptr(self.sums[2:]), L.ptr(self.ws),
                                       self.ws_bytes, _stream()), "bce")

    def backward_d_fake(self, grads, scale):
        """d(sum BCE(D(fake), 1) * scale)/d(fake) through the fake-half units (no parameter gradients: skip_wgrad)."""
        r = self.d_raw_fake
        L.check(self.lib.bp_bce_logits_grad(C.byref(r.view), 0, self.n, 1.0, scale, C.byref(r.grad), _stream()), "bce grad")
        for u in reversed(self.d_units_fake):
            u.backward(grads)
        self._join_side()

    def backward_d(self, grads, seed_real, seed_fake_target, fake_scale):
        """Seed d(loss)/d(logits): real half scale*(sigmoid-1) or 0; fake half with the given target."""
        lib, st, n, r = self.lib, _stream(), self.n, self.d_raw
        L.check(lib.bp_bce_logits_grad(C.byref(r.view), 0, n, 1.0, seed_real, C.byref(r.grad), st), "bce grad")
        L.check(lib.bp_bce_logits_grad(C.byref(r.view), n, 2 * n, seed_fake_target, fake_scale, C.byref(r.grad), st),
                "bce grad")
        for u in reversed(self.d_units):
            u.backward(grads)
        self._join_side()

    def backward_g(self, grads, l1_scale):
        lib, st = self.lib, _stream()
        L.check(lib.bp_tanh_l1_backward(C.byref(self.v_fake_x), L.ptr(self.x_nchw), C.byref(self.v_dfake), l1_scale,
                                        C.byref(self.g_raw.grad), st), "generator head backward")
        for u in reversed(self.g_units):
            u.backward(grads)
        self._join_side()

    def _join_side(self):
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)     # every weight gradient is written


class _GanPaintPlan(PlanBase):
    """The generator alone, eval mode only: what painting needs of a ``_GanPlan``.  No discriminator units, no
    ``prepare_backward`` (no gradient buffers, no weight-gradient workspace), no workspace at all (batch-norm runs on its
    running statistics: ``need_ws`` records the sizes and nothing is allocated), no side stream, and the data-gradient
    images of the packed weights are dropped.  The units are compiled exactly as ``_GanPlan`` compiles its generator
    (same names, same ``impl``), so the forward launches -- and the bits they produce -- are the same.

    ``paint_dtype="bf16"``: the 128-channel trunk runs on the bf16 matrix-core kernels and is stored as bf16 -- the last
    encoder (fp32 in, bf16 out), the residual blocks (bf16 throughout, their tails through bp_bf16_residual_forward) and
    the first decoder (bf16 in, fp32 out).  The k9 stem, the first encoder, the last decoder and the k9 head stay fp32.
    The two converted layers have a bias: in this eval-only plan it goes to the bf16 kernel with the forward call
    (``bf16_bias``; graph.ConvUnit turns bf16 off for a biased layer of any other plan)."""

    PAINT_DTYPES = ("fp32", "bf16")
    bf16_bias = True

    def __init__(self, model, n, paint_dtype="fp32"):
        if paint_dtype not in self.PAINT_DTYPES:
            raise ValueError(f"paint_dtype {paint_dtype!r}: one of {self.PAINT_DTYPES}")
        self.model, self.lib, self.device, self.impl, self.sync = model, model._lib, model.device, L.IMPL_AUTO, model.sync
        self.n, self.ws = n, None
        self.paint_dtype = paint_dtype
        self._bf16_units, self._bf16_outs = self.bf16_policy(model.g_arch) if paint_dtype == "bf16" else ((), ())
        H, W = model.tile_size, model.tile_size
        self.y2 = Slot.new(n, H, W, 2, self.device)
        gu, gs, tr = compile_sequential(self, "generator.", model.g_arch, model.generator, self.y2,
                                        need_input_grad=False)
        if [t[0] for t in tr] != ["tanh"]:
            raise NotImplementedError("the generator must end in conv + tanh")
        if gs.shape() != (n, H, W, 1) or gs.pw is not None:
            raise ValueError(f"generator output {gs.shape()}")
        self.g_units, self.g_raw = gu, gs
        self.units = self.flat_units(gu)
        for u in self.units:
            u.packed_bwd = None                   # (maybe_pack skips a direction that has no image)
        for u in self.units:
            want = self.bf16_unit(u.name)
            if want != u.bf16 or (want and self.lib.bp_conv_bf16_supported(
                    C.byref(u.cv), L.PACK_FWD, C.byref(u.inp.view), C.byref(u.out.view)) != 1):
                raise NotImplementedError(f"{u.name}: the bf16 kernels do not take this layer with these views")

    @staticmethod
    def bf16_policy(g_arch, prefix="generator."):
        """(name prefixes of the units that run in bf16, ... of those that also STORE bf16): the residual blocks, the
        convolution in front of the first one (it writes bf16) and the one behind the last (it reads bf16, writes fp32)."""
        names = [layer[0].lower() for layer in g_arch]
        res = [i for i, nm in enumerate(names) if nm == "residual block"]
        if not res or res != list(range(res[0], res[-1] + 1)):
            return (), ()
        convs = [i for i, nm in enumerate(names) if nm in ("conv", "transp conv")]
        enc, dec = max(i for i in convs if i < res[0]), min(i for i in convs if i > res[-1])
        outs = (f"{prefix}{enc}",) + tuple(f"{prefix}{i}.res_block." for i in res)
        return outs + (f"{prefix}{dec}",), outs

    @staticmethod
    def _named(name, keys):
        return any(name.startswith(k) if k.endswith(".") else name == k for k in keys)

    def bf16_unit(self, name):
        return self._named(name, self._bf16_units)

    def bf16_out(self, name):
        return self._named(name, self._bf16_outs)

    def forward(self):
        for u in self.g_units:
            u.forward(False)

    def generate(self, y, zc, out):
        """out (n, 1, H, W) = tanh(G(y, zc)): ``_GanPlan.generate`` + ``bp_view_to_nchw`` of the eval mode, the tanh
        written straight into ``out`` (one channel: NHWC with a stride of one IS NCHW)."""
        lib, st, n = self.lib, _stream(), self.n
        self._keep = (y.contiguous(), zc.reshape(n, 1).contiguous())
        L.check(lib.bp_nchw_to_view(L.ptr(self._keep[0]), 1, L.ptr(self._keep[1]), 1, C.byref(self.y2.view), st),
                "generator input")
        self.forward()
        ov = L.View(out.data_ptr(), n, self.g_raw.h, self.g_raw.w, 1, 1, 0, L.F32)
        L.check(lib.bp_unary_forward(C.byref(self.g_raw.view), None, 1, C.byref(ov), st), "tanh")


class CGAN(torch.nn.Module):
    """Generator + discriminator with their alternating training step."""

    def __init__(self, tile_size=512, device="cuda:0", n_res=9, lambda_perceptual=2.5, g_arch=None, d_arch=None,
                 sync=None, paint_dtype="fp32", train_dtype="fp32"):
        """``paint_dtype``: "fp32" or "bf16" -- the storage and matrix-core type of the 128-channel trunk in the
        INFERENCE plan (eval-mode ``generate``, ``paint_graph``; see ``_GanPaintPlan``).  Training ignores it.

        ``train_dtype``: "fp32" or "bf16" -- the same for the residual blocks of the TRAINING plan (``_GanPlan``: what runs
        in bf16 and where a tensor is rounded).  Independent of ``paint_dtype``; not available together with ``sync``.

        ``sync`` (baryon_painter_amd.dist.Sync): data parallel, one process per GPU -- the generator's batch-norm
        statistics become those of the global batch, the discriminator's and the generator's gradients are averaged
        over ranks as ONE flat buffer each, right after their backward pass (the spectral-norm power iteration is
        parameter-side arithmetic and identical on every rank)."""
        super().__init__()
        if train_dtype not in _GanPlan.TRAIN_DTYPES:
            raise ValueError(f"train_dtype {train_dtype!r}: one of {_GanPlan.TRAIN_DTYPES}")
        if train_dtype == "bf16" and sync is not None:
            raise NotImplementedError("train_dtype='bf16' is single-device: data-parallel bf16 CGAN training is not built")
        self.train_dtype = train_dtype
        self.sync = sync
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("baryon_painter_amd.CGAN runs on an AMD GPU only; there is no CPU implementation.")
        self._lib = L.load()
        if paint_dtype not in _GanPaintPlan.PAINT_DTYPES:
            raise ValueError(f"paint_dtype {paint_dtype!r}: one of {_GanPaintPlan.PAINT_DTYPES}")
        self.paint_dtype = paint_dtype
        self.tile_size = tile_size
        self.lambda_perceptual = lambda_perceptual
        self.g_arch = g_arch or cgan_generator_architecture(n_res)
        self.d_arch = d_arch or cgan_discriminator_architecture()
        self.generator = build_holders(self.g_arch)
        self.discriminator = build_holders(self.d_arch)
        self._init_weights()
        self.to(self.device)
        self.sn_layers = [m for m in self.discriminator if isinstance(m, SNConv2d)]
        self._plans = {}
        self._paint_plans = {}          # _paint_key(n) -> _GanPaintPlan (eval-mode generate, paint_graph)
        self._paint_graphs = {}         # _paint_key(n) -> the captured paint pipeline of paint_graph
        self._grads = {}
        self._flat = {}
        for name, net in (("d", self.discriminator), ("g", self.generator)):
            ps = list(net.parameters())
            flat = torch.zeros(sum(p.numel() for p in ps), device=self.device)
            off = 0
            for p in ps:
                p.grad = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
            self._flat[name] = flat
        for h in self.sn_layers:
            self._grads[id(h.weight)] = h.weight_grad
            h._grad_view = h.weight_orig.grad
        self._grad_pairs = [(p, p.grad) for p in self.parameters()]
        for p, gv in self._grad_pairs:
            self._grads[id(p)] = gv
        self.last = {}

    def _attach_grads(self):
        """``p.grad`` = the views of the flat gradient buffers the kernels write (and data parallelism averages) --
        re-attached at the start of every step: ``optimizer.zero_grad()`` / ``model.zero_grad()`` set them to None by
        default, and a gradient that lived outside the flat buffer would silently not be averaged across ranks."""
        for p, gv in self._grad_pairs:
            if p.grad is None or p.grad.data_ptr() != gv.data_ptr():
                p.grad = gv

    def _init_weights(self):
        """Kaiming-normal except the generator's last layer: Xavier with gain 0.25 (README.md:102)."""
        convs = [m for m in list(self.generator.modules()) + list(self.discriminator.modules())
                 if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
        last_g = [m for m in self.generator.modules() if isinstance(m, torch.nn.Conv2d)][-1]
        for m in convs:
            w = m.weight_orig if isinstance(m, SNConv2d) else m.weight
            if m is last_g:
                torch.nn.init.xavier_normal_(w, gain=0.25)
            else:
                torch.nn.init.kaiming_normal_(w, a=0.2)
            if m.bias is not None:
                torch.nn.init.zeros_(m.bias)

    def _plan(self, n):
        key = n if self.train_dtype == "fp32" else (n, self.train_dtype)
        if key not in self._plans:
            self._plans[key] = _GanPlan(self, n)
        return self._plans[key]

    def g_parameters(self):
        return list(self.generator.parameters())

    def d_parameters(self):
        return list(self.discriminator.parameters())

    @staticmethod
    def z_transform(z):
        return z - 1.0                                  # README.md:99

    def _inputs(self, y, z):
        y = torch.as_tensor(y, device=self.device, dtype=torch.float32)
        if y.dim() != 4 or tuple(y.shape[1:]) != (1, self.tile_size, self.tile_size):
            raise ValueError(f"y has shape {tuple(y.shape)}, model expects (N, 1, {self.tile_size}, {self.tile_size})")
        z = torch.as_tensor(z, device=self.device, dtype=torch.float32).reshape(-1)
        if z.numel() == 1 and y.shape[0] > 1:
            z = z.expand(y.shape[0])
        if z.shape[0] != y.shape[0]:
            raise ValueError("one redshift per sample")
        return y, self.z_transform(z)

    def _paint_key(self, n):
        """Key of the per-(n, paint_dtype) caches: ``n`` itself for fp32 (the key of before the dtype existed)."""
        return n if self.paint_dtype == "fp32" else (n, self.paint_dtype)

    def _paint_plan(self, n):
        key = self._paint_key(n)
        if key not in self._paint_plans:
            self._paint_plans[key] = _GanPaintPlan(self, n, self.paint_dtype)
        return self._paint_plans[key]

    def release_paint_buffers(self):
        """Free the inference plans and the captured paint graphs of both paint dtypes (they are rebuilt on the next
        use)."""
        self._paint_graphs.clear()
        self._paint_plans.clear()

    def generate(self, y, z):
        """G(dm, z) -> pressure in the network's (tanh) domain, (N,1,H,W).  In eval mode through the inference plan
        (generator units only); in training mode through the training plan, whose discriminator input it fills."""
        with torch.no_grad():
            y, zc = self._inputs(y, z)
            if not self.training:
                out = torch.empty((y.shape[0], 1, self.tile_size, self.tile_size), device=self.device)
                self._paint_plan(y.shape[0]).generate(y, zc, out)
                return out
            plan = self._plan(y.shape[0])
            plan.generate(y, zc, self.training)
            out = torch.empty((y.shape[0], 1, self.tile_size, self.tile_size), device=self.device)
            L.check(self._lib.bp_view_to_nchw(C.byref(plan.v_fake_x), None, 0, L.ptr(out), _stream()), "fake layout")
            return out

    # ---- hipGraph-captured paint pipeline: raw tiles in, physical tiles out
    def paint_graph(self, n):
        """The captured paint pipeline for batches of ``n`` RAW tiles, in the form of ``CVAE.paint_graph``: a dict with
        ``slots``: TWO input / parameter / output buffer sets, each with its own captured graph over the SAME inference
        plan (replay them on ONE stream).  A slot holds ``raw`` (n, 1, H, W) untransformed input tiles, ``out``
        (n, 1, H, W) painted physical tiles, ``block`` one uint8 device buffer with the typed views ``xf_in`` /
        ``xf_out`` (n, 3) float64 {sigma, k0, k1} / {k0, k1, sigma} of the shift-log-cam transform and its inverse and
        ``aux`` (n, 1) float32, the conditioning plane's value z - 1 (read by the kernel at run time: one graph serves
        every redshift), and ``graph``: bp_paint_load_cam -> generator units -> bp_paint_store_cam.  ``tile_ids`` and
        ``seed`` are part of the block (``block_layout``: name -> (byte offset, dtype, shape)) so that one caller fills
        either model's block; the generator has no latent noise and nothing reads them."""
        if self.training:
            raise RuntimeError("paint_graph is an eval-mode (paint) path: call model.train(False) first")
        g = self._paint_graphs.get(self._paint_key(n))
        if g is None:
            g = self._paint_graphs[self._paint_key(n)] = self._capture_paint_graph(n)
        for u in g["units"]:
            u.maybe_pack()                       # eager, a no-op unless the weights changed
            u.maybe_bn_eval()                    # ... or the running statistics
        return g

    def _capture_paint_graph(self, n):
        H = W = self.tile_size
        dev = self.device
        plan = self._paint_plan(n)
        block = PG.ParamBlock(PG.paint_fields(n, 3))
        st = {"param_block": block, "block_layout": block.layout, "block_bytes": block.nbytes, "plan": plan,
              "units": plan.units,
              "slots": [PG.new_slot((n, 1, H, W), (n, 1, H, W), block, dev) for _ in range(2)]}

        def run(sl):
            lib, sm = self._lib, _stream()
            L.check(lib.bp_paint_load_cam(L.ptr(sl["raw"]), 1, L.ptr(sl["xf_in"]), L.ptr(sl["aux"]), 1,
                                          C.byref(plan.y2.view), sm), "paint load")
            plan.forward()
            L.check(lib.bp_paint_store_cam(C.byref(plan.g_raw.view), L.ptr(sl["xf_out"]), L.ptr(sl["out"]), sm),
                    "paint store")

        PG.capture(run, st["slots"], dev)
        return st

    def train_step(self, x, y, z, opt_g, opt_d, capture=None):
        """One alternating iteration: D on (real, G(y).detach()), then G through the updated D.
        Returns the loss terms as device scalars (dict)."""
        with torch.no_grad():
            x = torch.as_tensor(x, device=self.device, dtype=torch.float32)
            y, zc = self._inputs(y, z)
            n = y.shape[0]
            plan = self._plan(n)
            self._attach_grads()
            plan.generate(y, zc, self.training)
            plan.load_real(x)
            return self._iterate(plan, opt_g, opt_d, capture)

    def train_step_assembled(self, fill, n, opt_g, opt_d, capture=None):
        """``train_step`` for a batch of ``n`` that is assembled on the device: ``fill(plan)`` writes the step's inputs
        straight into the training plan's buffers, through ``plan.fill`` (``_GanPlan.fill`` hands out the four
        destinations) -- e.g. ``lambda plan: assembler.gather_gan(indices, cam, aux, plan)``, one ``bp_gather_tiles_gan``
        launch (utils.datasets.DeviceTileAssembler) -- in place of the upload, the copies and the four layout launches of
        ``train_step``.  From there on the two methods run the same function: the same inputs give the same bits.
        Returns the loss terms as device scalars."""
        with torch.no_grad():
            plan = self._plan(int(n))
            self._attach_grads()
            fill(plan)
            plan.forward_g(self.training)
            return self._iterate(plan, opt_g, opt_d, capture)

    def _iterate(self, plan, opt_g, opt_d, capture):
        """The alternating iteration over a plan whose inputs are in place and whose generator has run."""
        with torch.no_grad():
            # ---- discriminator step
            plan.discriminate(self.training)
            plan.d_losses()
            plan.backward_d(self._grads, 0.5 / plan.cnt_d, 0.0, 0.5 / plan.cnt_d)
            for h in self.sn_layers:
                h.finish_backward()
            loss_d = 0.5 * (plan.sums[0] + plan.sums[1]) / plan.cnt_d
            if self.sync is not None:
                self.sync.all_reduce_mean(self._flat["d"])
            if capture is not None:        # tests: gradients of the discriminator step
                capture["d"] = {k: p.grad.clone() for k, p in self.discriminator.named_parameters()}
            opt_d.step()
            # ---- generator step (same fake, updated discriminator)
            plan.discriminate(self.training, fake_only=True)
            plan.g_adv_loss()
            lib, st = self._lib, _stream()
            L.check(lib.bp_l1_sum(C.byref(plan.v_fake_x), L.ptr(plan.x_nchw), L.ptr(plan.sums[3:]), L.ptr(plan.ws),
                                  plan.ws_bytes, st), "l1")
            plan.skip_wgrad = True          # through D only for d(loss)/d(fake): its parameters do not step here
            try:
                plan.backward_d_fake(self._grads, 0.5 / plan.cnt_d)
            finally:
                plan.skip_wgrad = False
            plan.backward_g(self._grads, self.lambda_perceptual / plan.cnt_px)
            loss_g_adv = 0.5 * plan.sums[2] / plan.cnt_d
            loss_g_perc = plan.sums[3] / plan.cnt_px
            if self.sync is not None:
                self.sync.all_reduce_mean(self._flat["g"])
            if capture is not None:
                capture["g"] = {k: p.grad.clone() for k, p in self.generator.named_parameters()}
            opt_g.step()
            self.last = {"D": loss_d, "G_adv": loss_g_adv, "G_perceptual": loss_g_perc}
            return self.last
