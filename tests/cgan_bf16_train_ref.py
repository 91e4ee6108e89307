"""Float64 ROUNDING TWIN of one CGAN training iteration under ``train_dtype="bf16"`` (TEST INFRASTRUCTURE).

Truth is ``oracle.cgan_torch.TorchCGAN(dtype=torch.float64)``.  The twin is the same iteration -- the same class, the
same losses, optimizers and discriminator -- whose generator is the float64 graph with a tensor rounded to bf16 (value on
the way forward, gradient on the way back: ``oracle.torch_ref._StoreBf16``) at exactly the points the training plan's
docstring lists (baryon_painter_amd/models/cgan.py, ``_GanPlan``):

  * the entry cast: A0 = leaky(batchnorm(raw)) of the last encoder, rounded once; operand of the first block's first
    convolution and that block's skip; its gradient -- the sum of both consumers -- rounded once;
  * the residual convolutions' weights (value only: the weight gradients are fp32);
  * their staged activated inputs, and the data gradients stored in those slots;
  * their stored raw outputs and d(loss)/d(raw);
  * every block's output and its gradient;
  * the exit cast: the value passes exactly, the decoder's data gradient is rounded once (the block output's rounding).

The layers in front of the entry and behind the exit, the discriminator and the losses are not rounded.  Built on
tests/cgan_bf16_ref.py's conventions; like that twin it is not bit-equal to the kernels (accumulation order, fp32 against
float64): it shows what a correct bf16 execution's distance from the truth is, per tensor, at this network's conditioning.
"""
import torch.nn.functional as F

import oracle.cgan_torch as CT
from oracle.torch_ref import _StoreBf16, _seq

from cgan_bf16_ref import bf16_layers


def twin_generator(g_arch, x, P, prefix, training):
    """``oracle.torch_ref._seq`` of the generator's layer list with the training plan's roundings."""
    enc, res, dec = bf16_layers(g_arch)
    # ``_seq`` numbers layers from zero: the layers in front of the first block as they are ...
    x = _seq(g_arch[:res[0]], x, P, prefix, training)
    x = _StoreBf16.apply(x, True)                                               # entry
    for i in res:
        body, (tail, slope) = g_arch[i][1]
        assert tail.lower() == "leaky relu"
        p = f"{prefix}{i}.res_block."
        # every convolution of the body: (bf16 matrix cores, output stored as bf16, input slot is bf16)
        policy = {f"{p}{j}": (True, True, True) for j, layer in enumerate(body) if layer[0].lower() == "conv"}
        h = _seq(body, x, P, p, training, bf16=policy) + x
        x = _StoreBf16.apply(F.leaky_relu(h, slope), True)                      # block output (the last one: the exit)
    # ... and those behind the last block under their own indices
    return _seq([("leaky relu", 1.0)] * dec + list(g_arch[dec:]), x, P, prefix, training)


class TwinCGAN(CT.TorchCGAN):
    """``TorchCGAN`` whose ``iteration`` runs ``twin_generator`` where the parent runs ``_seq`` on the generator."""

    def iteration(self, *args, **kwargs):
        def seq(arch, x, P, prefix, training, *a, **k):
            assert prefix == "generator." and not a and not k
            return twin_generator(arch, x, P, prefix, training)
        keep, CT._seq = CT._seq, seq
        try:
            return super().iteration(*args, **kwargs)
        finally:
            CT._seq = keep
