"""GPU: a weight-gradient call that qualifies differently from its workspace query still fits the queried bytes.

tests/golden/wgrad_dispatch.json pins what the dispatcher plans and how many bytes the workspace query grants; what a
table cannot show is the call whose kernel is another than the one the query saw.  Two things do that (csrc/kernels.hpp,
WgradFamily::may_requalify): bp_set_option switches a trunk layer between its output-stationary kernel and the tiled
one after the workspace was sized, and the call carries a pointwise operand, which the query never sees.  Each case
here queries first, then runs with a workspace of exactly the queried bytes filled with NaN and followed by a 256-byte
guard that must stay NaN, on the integer data of tests/wgrad_sweep.py: dW equals the float64 reference exactly.

Through bp_conv_backward_weight a pointwise operand cannot move a layer: it lands on Y only for a transposed layer, the
stem and flat kernels take plain convolutions only, and flat_s2 refuses only operands on both sides.  So the pointwise
cases are flat_s2's transposed layer with and without x_pw -- the same family, the kernel instantiation that applies the
operand on the half-resolution side and the one that does not.  (test_gpu_wgrad_sweep.py runs that layer with x_pw at
the extents where a split walks several tiles.)
"""
import ctypes as C

import pytest
import torch

from baryon_painter_amd import _lib as L

import conv_sweep as S
import gpu_util as G
import wgrad_sweep as W

pytestmark = pytest.mark.gpu

GUARD = 256
TRUNK = (0, 128, 128, 3, 1, 1, 0)
FLAT_S2_T = (1, 32, 16, 4, 2, 1, 0)


def _view(t, bf16):
    """An NHWC tensor as a 16-byte addressable channel slice of a wider buffer."""
    n, h, w, c = t.shape
    cs, co = W.layout(c, "aligned", bf16)
    buf = torch.full((n, h, w, cs), 7.5, dtype=torch.float32, device="cuda")
    buf[..., co:co + c] = t
    if bf16:
        buf = buf.to(torch.bfloat16)
    return buf, L.View(buf.data_ptr(), n, h, w, c, cs, co, L.BF16 if bf16 else L.F32)


def _family(lib, cv, xv, dyv, flag):
    out = (C.c_int32 * 4)()
    assert lib.bp_conv_backward_weight_plan(C.byref(cv), C.byref(xv), C.byref(dyv), flag, out) == L.BP_OK
    return L.WGRAD_FAMILIES[out[0]]


class Layer:
    def __init__(self, case, index, bf16):
        self.lib, self.case, self.bf16 = L.load(), case, bf16
        self.cv = L.Conv(*case[:7])
        self.flag = L.IMPL_BF16 if bf16 else L.IMPL_MFMA
        self.x, self.dy, self.pw_host = W.int_inputs(case, index, "cuda")
        assert W.magnitude_bound(self.dy, self.pw_host) < W.EXACT_LIMIT
        self.keep, self.pw = G.pointwise(*(v.numpy() for v in self.pw_host))
        (self.xb, self.xv), (self.dyb, self.dyv) = _view(self.x, bf16), _view(self.dy, bf16)

    def query(self):
        nb = self.lib.bp_conv_backward_weight_workspace(C.byref(self.cv), C.byref(self.xv), C.byref(self.dyv))
        assert nb > 0 and nb % 4 == 0
        return nb

    def family(self):
        return _family(self.lib, self.cv, self.xv, self.dyv, self.flag)

    def run_exact(self, nb, with_pw, what):
        """One call with exactly nb bytes of NaN workspace: BP_OK, the guard untouched, dW exact."""
        ws = torch.full(((nb + GUARD) // 4,), float("nan"), device="cuda")
        dw = torch.full(S.weight_shape(self.case), float("nan"), device="cuda")
        rc = self.lib.bp_conv_backward_weight(C.byref(self.cv), C.byref(self.xv), C.byref(self.pw) if with_pw else None,
                                              C.byref(self.dyv), L.ptr(dw), None, L.ptr(ws), nb, self.flag, G.stream())
        assert rc == L.BP_OK, "%s: returned %d (%s)" % (what, rc, self.lib.bp_strerror(rc).decode())
        assert bool(torch.isnan(ws[nb // 4:]).all()), "%s: stores behind the workspace" % what
        xa = W.activated(self.x, self.pw_host, self.bf16) if with_pw else self.x.double()
        ref = W.reference_dw(self.case, xa, self.dy.double())
        got = dw.double()
        bad = int((got != ref).sum())
        assert bad == 0, "%s: %d of %d elements differ from the float64 reference of the integer data" % (what, bad, ref.numel())


@pytest.mark.parametrize("option,bf16,extent,on,off", [
    (b"f32_wgrad_ws", False, (1, 8, 16), "ws_f32", ("tiles", "tiles_dma")),
    (b"bf16_wgrad_ws", True, (1, 8, 32), "ws_bf16", ("bf16_tiled",)),
], ids=["ws_f32", "ws_bf16"])
def test_trunk_layer_switched_to_the_tiled_kernel_after_its_workspace_query(option, bf16, extent, on, off):
    layer = Layer(TRUNK + extent, 1, bf16)
    lib = layer.lib
    try:
        assert lib.bp_set_option(option, 1) == 0
        nb = layer.query()
        assert layer.family() == on
        assert lib.bp_set_option(option, 0) == 0
        assert layer.family() in off
        layer.run_exact(nb, True, "%s -> %s" % (on, off[0]))
    finally:
        lib.bp_set_option(option, -1)


@pytest.mark.parametrize("with_pw", [False, True], ids=["plain", "x_pw"])
def test_transposed_flat_s2_layer_with_and_without_its_pointwise_operand(with_pw):
    # the smallest extent tests/golden/wgrad_dispatch.json records under flat_s2 for this layer (gate:flat_t4_32_16):
    # four workgroups, none with a whole tile
    layer = Layer(FLAT_S2_T + (2, 5, 7), 2, False)
    assert layer.family() == "flat_s2"
    layer.run_exact(layer.query(), with_pw, "flat_s2 transposed, %s" % ("x_pw on Y" if with_pw else "no pointwise operand"))
