"""GPU: the two kernels ``train_dtype="bf16"`` of the CGAN adds -- the column strips of the output-stationary bf16 weight
gradient (conv_wgrad_ws_bf16.hip, widths 128 / 192 / 256) and bp_view_cast (pointwise_bf16.hip).

Strip weight gradient, by the method of tests/wgrad_sweep.py: small-integer data (dY in {-1, 0, 1}, the activated X in
quarter units) whose sums of |products| stay below 2^24 quarter-units, so every order of fp32 accumulation is exact and
the device dW must EQUAL the float64 reference -- a pixel dropped at a seam, counted twice or taken from the wrong strip
shows as a difference of at least 1/4.  Cases: one, two, four, eight and sixteen bands per image, two, three and four
strips (tests/test_cgan_bf16_train_host.py pins those counts), with and without a pending pointwise, aligned views and
views with channel stride 136 and offset 8; the seams and the image edge on their own; the same bits twice; the tiled
kernel (option off) on the same data.

bp_view_cast against NumPy: round to nearest even on bits, the 16-byte and the scalar path.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import gpu_util as G
from wgrad_sweep import EXACT_LIMIT, activated, int_inputs, magnitude_bound, reference_dw

pytestmark = pytest.mark.gpu

TRUNK = (0, 128, 128, 3, 1, 1, 0)
CASES = [(1, 1, 128), (2, 9, 128), (3, 20, 192), (2, 37, 256), (1, 128, 128)]
LAYOUTS = [(128, 0), (136, 8)]          # (channel stride, channel offset)
GUARD = 256


def _operand(t, layout, poison=7.5):
    """NHWC float tensor -> bf16 buffer with one pixel row in front of and behind the tensor and `layout`'s channels around
    the window, all poisoned; the view of the window."""
    n, h, w, c = t.shape
    cs, co = layout
    buf = torch.full((n * h + 2, w, cs), poison, dtype=torch.float32, device="cuda")
    buf[1:-1].view(n, h, w, cs)[..., co:co + c] = t
    buf = buf.to(torch.bfloat16)
    return buf, L.View(buf[1].data_ptr(), n, h, w, c, cs, co, L.BF16)


def _plan(lib, cv, xv, dyv):
    out = (C.c_int32 * 4)()
    assert lib.bp_conv_backward_weight_plan(C.byref(cv), C.byref(xv), C.byref(dyv), L.IMPL_BF16, out) == L.BP_OK
    return L.WGRAD_FAMILIES[out[0]], out[1]


def _call(lib, cv, xv, pw, dyv):
    """One bp_conv_backward_weight on NaN-filled dW and workspace: dW (the guard behind the workspace checked)."""
    nb = lib.bp_conv_backward_weight_workspace(C.byref(cv), C.byref(xv), C.byref(dyv))
    assert nb > 0 and nb % 4 == 0
    ws = torch.full(((nb + GUARD) // 4,), float("nan"), device="cuda")
    dw = torch.full((128, 128, 3, 3), float("nan"), device="cuda")
    rc = lib.bp_conv_backward_weight(C.byref(cv), C.byref(xv), C.byref(pw) if pw is not None else None, C.byref(dyv),
                                     L.ptr(dw), None, L.ptr(ws), nb, L.IMPL_BF16, G.stream())
    assert rc == L.BP_OK, lib.bp_strerror(rc).decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nb // 4:]).all()), "stores behind the workspace"
    return dw


def _exact(what, got, ref):
    got = got.double()
    if not torch.equal(got, ref):
        bad = got != ref
        worst = (got - ref)[bad].abs().max().item() if not torch.isnan(got).any() else float("nan")
        pytest.fail("%s: %d of %d elements differ from the float64 reference of the integer data (largest difference %s)"
                    % (what, int(bad.sum()), ref.numel(), worst))


@functools.lru_cache(maxsize=None)
def _data(nhw, with_pw):
    """(x, dy, pointwise tensors or None, float64 reference dW) of a case: computed once, shared, never written."""
    case = TRUNK + nhw
    x, dy, pw_host = int_inputs(case, CASES.index(nhw), "cuda")
    if not with_pw:
        pw_host = None
        bound = 4.0 * 2.0 * float(dy.abs().double().sum(dim=(0, 1, 2)).max())       # |x| <= 2
        xa = x.double()
    else:
        bound = magnitude_bound(dy, pw_host)
        xa = activated(x, pw_host, round_bf16=True)
        assert torch.equal(xa, activated(x, pw_host)), "the activated integers are exact in bf16"
    assert bound < EXACT_LIMIT, (nhw, bound)
    return x, dy, pw_host, reference_dw(case, xa, dy.double())


@pytest.mark.parametrize("with_pw", [False, True], ids=["raw", "pointwise"])
@pytest.mark.parametrize("nhw", CASES, ids=["%dx%dx%d" % c for c in CASES])
def test_strip_weight_gradient_equals_the_float64_reference(nhw, with_pw):
    lib = L.load()
    cv = L.Conv(*TRUNK)
    x, dy, pw_host, ref = _data(nhw, with_pw)
    keep, pw = G.pointwise(*(v.numpy() for v in pw_host)) if with_pw else (None, None)
    for layout in LAYOUTS:
        what = "%s stride %d offset %d" % ((nhw,) + layout)
        xb, xv = _operand(x, layout)
        yb, dyv = _operand(dy, layout)
        family, ns = _plan(lib, cv, xv, dyv)
        assert family == "ws_bf16", what
        dw = _call(lib, cv, xv, pw, dyv)
        _exact(what + " strips", dw, ref)
        assert torch.equal(dw, _call(lib, cv, xv, pw, dyv)), what + ": the second call gave other bits"
        try:                                            # the tiled kernel on the same data
            assert lib.bp_set_option(b"BP_BF16_WGRAD_WS", 0) == L.BP_OK
            assert _plan(lib, cv, xv, dyv)[0] == "bf16_tiled", what
            tiled = _call(lib, cv, xv, pw, dyv)
        finally:
            lib.bp_set_option(b"BP_BF16_WGRAD_WS", -1)
        _exact(what + " tiled", tiled, ref)
        assert torch.equal(tiled, dw), what


def _column_pair(n, h, w, x_col, y_col):
    x = torch.zeros((n, h, w, 128), device="cuda")
    dy = torch.zeros((n, h, w, 128), device="cuda")
    c = torch.arange(128, device="cuda", dtype=torch.float32)
    x[:, :, x_col] = 1.0 + (c % 3)                      # 1, 2, 3: every channel pair gives a non-zero product
    dy[:, :, y_col] = 1.0 - 2.0 * (c % 2)
    return x, dy


@pytest.mark.parametrize("poison", [7.5, float("nan")], ids=["seam", "edge"])
def test_only_the_taps_that_read_across_a_seam_are_non_zero(poison):
    """192 pixels = three strips, seams in front of columns 64 and 128.  X lives in the column right of a seam and dY in
    the column left of it (then the other way round): dW is non-zero in exactly the taps kx = 2 (kx = 0) -- the strip that
    owns dY's column reads the activation from its neighbour's column, through its halo.  `edge`: the same with NaN in
    every channel outside the window and in the pixel rows in front of and behind the tensor: none reaches dW (an
    out-of-image row, or a halo column at the image edge, is loaded from a valid address and masked to zero)."""
    lib = L.load()
    cv = L.Conv(*TRUNK)
    n, h, w = 2, 3, 192
    case = TRUNK + (n, h, w)
    for seam in (64, 128):
        for x_col, y_col, kx in ((seam, seam - 1, 2), (seam - 1, seam, 0)):
            x, dy = _column_pair(n, h, w, x_col, y_col)
            ref = reference_dw(case, x.double(), dy.double())
            want = torch.zeros((128, 128, 3, 3), dtype=torch.bool, device="cuda")
            want[:, :, :, kx] = True
            assert torch.equal(ref != 0, want)
            for layout in LAYOUTS:
                xb, xv = _operand(x, layout, poison)
                yb, dyv = _operand(dy, layout, poison)
                assert _plan(lib, cv, xv, dyv) == ("ws_bf16", n * 1 * 3)
                dw = _call(lib, cv, xv, None, dyv)
                assert torch.equal(dw != 0, want), (seam, x_col, layout)
                _exact("seam %d x %d" % (seam, x_col), dw, ref)
    # the image's own edge columns: X in column 0 / w - 1, dY beside it -- nothing wraps into the next row or image
    for x_col, y_col, kx in ((0, 1, 0), (w - 1, w - 2, 2), (0, 0, 1), (w - 1, w - 1, 1)):
        x, dy = _column_pair(n, h, w, x_col, y_col)
        ref = reference_dw(case, x.double(), dy.double())
        xb, xv = _operand(x, LAYOUTS[1], poison)
        yb, dyv = _operand(dy, LAYOUTS[1], poison)
        dw = _call(lib, cv, xv, None, dyv)
        assert torch.equal(dw[:, :, :, [j for j in range(3) if j != kx]], torch.zeros((128, 128, 3, 2), device="cuda"))
        _exact("edge column %d" % x_col, dw, ref)


# ---------------------------------------------------------------------------------------------------- bp_view_cast
def _bf16_bits(a):
    """uint16 bit patterns of float32 values rounded to bf16, to nearest even (finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _cast_data(shape, seed):
    """Multiples of 1/64 in [-4, 4], scales {1/2, 1, 3/2, 2}, shifts multiples of 1/8, slopes {1/4, 1/2, 0}: scale * x + shift
    and the slope's product are exact in fp32 however they are evaluated, and carry up to 12 significant bits -- four more
    than bf16 keeps."""
    rng = np.random.Generator(np.random.PCG64([77, seed]))
    c = shape[-1]
    x = (rng.integers(-256, 257, shape) / 64.0).astype(np.float32)
    scale = np.array([0.5, 1.0, 1.5, 2.0], np.float32)[rng.integers(0, 4, c)]
    shift = (rng.integers(-8, 9, c) / 8.0).astype(np.float32)
    slope = np.array([0.25, 0.5, 0.0], np.float32)[np.arange(c) % 3]
    return x, scale, shift, slope


def _np_pointwise(x, scale, shift, slope):
    t = x.astype(np.float64) * scale + shift
    return np.where(t > 0, t, t * slope).astype(np.float32)


# (n, h, w, c, source (stride, offset), destination (stride, offset))
CAST_SHAPES = [
    (3, 5, 7, 128, (128, 0), (128, 0)),             # 16 bytes per lane
    (2, 40, 33, 128, (136, 8), (128, 0)),           # ... several workgroups, a strided source
    (3, 5, 7, 24, (32, 8), (40, 16)),               # ... three units per pixel: a thread's channels change per trip
    (3, 5, 7, 3, (7, 2), (7, 3)),                   # ragged: the scalar path
    (3, 4, 5, 128, (132, 4), (128, 0)),             # a stride that is no multiple of 8: the scalar path
    (1, 1, 1, 128, (128, 0), (128, 0)),             # one pixel
    (1, 1, 1, 3, (7, 2), (3, 0)),
]


@pytest.mark.parametrize("with_pw", [False, True], ids=["plain", "pointwise"])
@pytest.mark.parametrize("shape", CAST_SHAPES, ids=["%dx%dx%dx%d-%s-%s" % s for s in CAST_SHAPES])
def test_view_cast_to_bf16_rounds_to_nearest_even(shape, with_pw):
    lib = L.load()
    n, h, w, c, (scs, sco), (dcs, dco) = shape
    x, scale, shift, slope = _cast_data((n, h, w, c), c)
    flat = x.reshape(-1)
    flat[:4] = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -0.75][:flat.size]     # two ties, a negative input
    src = torch.full((n, h, w, scs), float("nan"), device="cuda")
    src[..., sco:sco + c] = torch.from_numpy(x).cuda()
    dst = torch.full((n, h, w, dcs), -3.0, device="cuda").to(torch.bfloat16)
    sv = L.View(src.data_ptr(), n, h, w, c, scs, sco, L.F32)
    dv = L.View(dst.data_ptr(), n, h, w, c, dcs, dco, L.BF16)
    keep, pw = G.pointwise(scale, shift, slope) if with_pw else (None, None)
    assert lib.bp_view_cast(C.byref(sv), C.byref(pw) if with_pw else None, C.byref(dv), G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    want = _bf16_bits(_np_pointwise(x, scale, shift, slope) if with_pw else x)
    got = dst.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got[..., dco:dco + c], want)
    if not with_pw and flat.size >= 3:           # 1 + 2^-8 -> 1 (even), 1 + 3 2^-8 -> 1 + 2^-6 (even)
        assert list(want.reshape(-1)[:3]) == [0x3F80, 0x3F82, 0xBF80]
    outside = np.ones(dcs, bool)
    outside[dco:dco + c] = False
    assert (got[..., outside] == 0xC040).all(), "channels outside the window were written"       # bf16(-3)


@pytest.mark.parametrize("shape", CAST_SHAPES, ids=["%dx%dx%dx%d-%s-%s" % s for s in CAST_SHAPES])
def test_view_cast_to_fp32_is_exact(shape):
    lib = L.load()
    n, h, w, c, (scs, sco), (dcs, dco) = shape
    rng = np.random.Generator(np.random.PCG64([78, c]))
    bits = rng.integers(0, 1 << 16, (n, h, w, c)).astype(np.uint16)
    bits[(bits & 0x7F80) == 0x7F80] &= 0xBFFF                  # (no infinities or NaNs: compared as numbers below)
    src = torch.full((n, h, w, scs), float("nan"), device="cuda").to(torch.bfloat16)
    src.view(torch.int16)[..., sco:sco + c] = torch.from_numpy(bits.view(np.int16)).cuda()
    dst = torch.full((n, h, w, dcs), -3.0, device="cuda")
    sv = L.View(src.data_ptr(), n, h, w, c, scs, sco, L.BF16)
    dv = L.View(dst.data_ptr(), n, h, w, c, dcs, dco, L.F32)
    assert lib.bp_view_cast(C.byref(sv), None, C.byref(dv), G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    got = dst.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[..., dco:dco + c], bits.astype(np.uint32) << 16)
    outside = np.ones(dcs, bool)
    outside[dco:dco + c] = False
    assert (dst.cpu().numpy()[..., outside] == -3.0).all()


def test_view_cast_refuses_equal_types_and_different_shapes():
    lib = L.load()
    a = torch.zeros((2, 3, 4, 8), device="cuda")
    b = torch.zeros((2, 3, 4, 8), device="cuda", dtype=torch.bfloat16)
    va = L.View(a.data_ptr(), 2, 3, 4, 8, 8, 0, L.F32)
    vb = L.View(b.data_ptr(), 2, 3, 4, 8, 8, 0, L.BF16)
    assert lib.bp_view_cast(C.byref(va), None, C.byref(va), G.stream()) == L.BP_EINVAL
    assert lib.bp_view_cast(C.byref(vb), None, C.byref(vb), G.stream()) == L.BP_EINVAL
    for other in (L.View(b.data_ptr(), 2, 3, 4, 4, 8, 0, L.BF16), L.View(b.data_ptr(), 2, 3, 2, 8, 8, 0, L.BF16),
                  L.View(b.data_ptr(), 1, 3, 4, 8, 8, 0, L.BF16)):
        assert lib.bp_view_cast(C.byref(va), None, C.byref(other), G.stream()) == L.BP_EINVAL
    assert lib.bp_view_cast(C.byref(va), None, C.byref(vb), G.stream()) == L.BP_OK
    torch.cuda.synchronize()
