"""GPU: column strips of the weights-stationary bf16 k3 kernel (csrc/conv_bf16_ws.hip, kind 3) at the widths of the
CGAN generator's trunk: images wider than 64 pixels are cut into 64-pixel strips whose pad columns hold the neighbouring
strips' pixels (zeros where the image ends).

Same yardstick as tests/test_gpu_bf16_ops.py::test_weights_stationary_kernels: operands rounded to bf16, the float64
convolution of oracle/ops.py as truth, views that are channel slices of NaN-filled buffers, the three activation modes,
forward (with and without the batch-norm sums) and data gradient, the tiled kernel (bp_set_option("bf16_ws", 0)) beside
the stationary one.  The limits are that test's: 4e-3 of the tensor's scale against float64 for both kernels, 8e-3
between the kernels with fewer than 5 % of the elements different, and NOT bit-equal (which would mean the stationary
kernel never ran).

A strip seam is tested with numbers that are exact in bf16 at every step, so that a missing or stale halo column is a
wrong number and not a rounding difference, and with a NaN that has to cross the seam."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L
from oracle import ops

import gpu_util as G

pytestmark = pytest.mark.gpu

CI = CO = 128
CONV = (0, CI, CO, 3, 1, 1, 0)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def to_view(x_nchw, cstride, coff):
    """NCHW numpy -> bf16 NHWC view that is a channel slice of a NaN-filled buffer."""
    n, c, h, w = x_nchw.shape
    buf = torch.full((n, h, w, cstride), float("nan"), dtype=torch.float32, device="cuda")
    buf[..., coff:coff + c] = torch.from_numpy(np.ascontiguousarray(x_nchw.transpose(0, 2, 3, 1))).cuda()
    buf = buf.to(torch.bfloat16)
    return buf, L.View(buf.data_ptr(), n, h, w, c, cstride, coff, L.BF16)


def empty_view(n, h, w, c, cstride, coff):
    buf = torch.full((n, h, w, cstride), float("nan"), dtype=torch.bfloat16, device="cuda")
    return buf, L.View(buf.data_ptr(), n, h, w, c, cstride, coff, L.BF16)


def from_view(buf, c, coff):
    return buf[..., coff:coff + c].to(torch.float32).permute(0, 3, 1, 2).contiguous().cpu().numpy()


def outside_is_nan(buf, c, coff):
    raw = buf.to(torch.float32)
    return bool(torch.isnan(raw[..., :coff]).all() and torch.isnan(raw[..., coff + c:]).all())


def activate(x, act, scale, shift, slope):
    """The staging's arithmetic: fmaf in fp32 (the product is exact in float64: one rounding), leaky ReLU, bf16."""
    if act == "none":
        return x.astype(np.float64)
    t = (x.astype(np.float64) * scale[None, :, None, None].astype(np.float64)
         + shift[None, :, None, None].astype(np.float64)).astype(np.float32)
    return bf16_round(np.where(t > 0, t, t * slope[None, :, None, None]).astype(np.float32)).astype(np.float64)


def packed(lib, cv, wd, st):
    pf = torch.zeros(lib.bp_conv_bf16_packed_elems(C.byref(cv), L.PACK_FWD), device="cuda", dtype=torch.bfloat16)
    pb = torch.zeros(lib.bp_conv_bf16_packed_elems(C.byref(cv), L.PACK_BWD), device="cuda", dtype=torch.bfloat16)
    L.check(lib.bp_conv_bf16_pack(C.byref(cv), L.PACK_FWD, L.ptr(wd), L.ptr(pf), st))
    L.check(lib.bp_conv_bf16_pack(C.byref(cv), L.PACK_BWD, L.ptr(wd), L.ptr(pb), st))
    return pf, pb


# (n, h, w): the smallest shapes that reach every strip case
SHAPES = [
    ((1, 5, 128), ("none", "relu", "leaky")),       # two strips, a band that ends inside the image
    ((2, 9, 128), ("none", "relu", "leaky")),       # two strips, several band sizes
    ((3, 4, 192), ("none", "relu", "leaky")),       # three strips: the middle one has a neighbour on both sides
    ((1, 128, 128), ("leaky",)),                    # the CGAN's own trunk image, once
    ((70, 4, 128), ("none", "relu", "leaky")),      # many images, whole-image bands
    ((2, 9, 64), ("none", "relu", "leaky")),        # unchanged width: one strip, the kernel of before
    ((1, 4, 256), ("leaky",)),                      # the widest the kernel takes: four strips
]


@functools.lru_cache(maxsize=None)
def problem(shape, act):
    """Operands and the float64 truth of one case, computed once."""
    n, h, w = shape
    rng = np.random.default_rng(n * 1000 + h * 10 + w + 3)
    x = bf16_round(rng.standard_normal((n, CI, h, w)).astype(np.float32))
    wt = (rng.standard_normal((CO, CI, 3, 3)) * 0.05).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, CI).astype(np.float32)
    shift = rng.uniform(0.2, 0.6, CI).astype(np.float32)          # act(0) != 0: padding must stay 0
    slope = rng.uniform(0.0, 0.3, CI).astype(np.float32)
    if act == "relu":
        slope[:] = 0.0
    w64 = bf16_round(wt).astype(np.float64)
    y_ref = ops.conv2d_fwd(activate(x, act, scale, shift, slope), w64, 1, 1)
    dy = bf16_round(rng.standard_normal(y_ref.shape).astype(np.float32))
    dx_ref = ops.conv2d_bwd_data(dy.astype(np.float64), w64, 1, 1, h, w)
    for a in (x, wt, scale, shift, slope, y_ref, dy, dx_ref):
        a.setflags(write=False)
    return x, wt, scale, shift, slope, y_ref, dy, dx_ref


@pytest.mark.parametrize("shape,act", [(sh, a) for sh, acts in SHAPES for a in acts],
                         ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_strip_kernel_forward_and_data_gradient(shape, act):
    lib = L.load()
    n, h, w = shape
    x, wt, scale, shift, slope, y_ref, dy, dx_ref = problem(shape, act)
    cv = L.Conv(*CONV)
    st = G.stream()
    xb, xv = to_view(x, CI + 16, 8)
    keep, pw = G.pointwise(scale, shift, slope)
    pwp = None if act == "none" else C.byref(pw)
    wd = G.dev(wt)
    pf, pb = packed(lib, cv, wd, st)
    dyb, dyv = to_view(dy, CO + 16, 8)
    res = {}
    try:
        for ws_on in (1, 0):
            assert lib.bp_set_option(b"bf16_ws", ws_on) == 0
            yb, yv = empty_view(n, h, w, CO, CO + 8, 8)
            dxb, dxv = empty_view(n, h, w, CI, CI + 8, 0)
            for d, vi, vo in ((L.PACK_FWD, xv, yv), (L.PACK_BWD, dyv, dxv)):
                assert lib.bp_conv_ws_kind(C.byref(cv), d, C.byref(vi), C.byref(vo)) == (3 if ws_on else 0)
            L.check(lib.bp_conv_forward(C.byref(cv), C.byref(xv), pwp, L.ptr(pf), L.ptr(wd), None, C.byref(yv),
                                        L.IMPL_BF16, st), "forward")
            got = from_view(yb, CO, 8)
            e = G.rel_err(got, y_ref)
            print("forward ws=%d rel_err %.3e" % (ws_on, e))
            assert e < 4e-3, f"forward ws={ws_on}"
            assert outside_is_nan(yb, CO, 8), "stores outside the view"
            # ---- with the batch-norm sums (mode 1), where the layer accepts it: the sums of the tensor AS STORED
            nb = lib.bp_conv_stats_workspace(C.byref(cv), L.PACK_FWD, C.byref(xv), C.byref(yv), L.IMPL_BF16)
            if nb > 0:
                yb2, yv2 = empty_view(n, h, w, CO, CO + 8, 8)
                sums = torch.full((2 * CO,), float("nan"), dtype=torch.float64, device="cuda")
                wss = torch.full((nb // 8 + 8,), float("nan"), dtype=torch.float64, device="cuda")
                L.check(lib.bp_conv_forward_stats(C.byref(cv), C.byref(xv), pwp, L.ptr(pf), C.byref(yv2), L.ptr(sums),
                                                  L.ptr(wss), nb, L.IMPL_BF16, st), "forward + statistics")
                assert np.array_equal(from_view(yb2, CO, 8), got), "the statistics epilogue must not change the output"
                g64 = got.astype(np.float64)
                sm = sums.cpu().numpy()
                assert (np.abs(sm[:CO] - g64.sum(axis=(0, 2, 3))) <= 1e-6 * np.abs(g64).sum(axis=(0, 2, 3)) + 1e-12).all()
                assert np.allclose(sm[CO:], (g64 ** 2).sum(axis=(0, 2, 3)), rtol=1e-6, atol=1e-12)
            else:
                assert not ws_on, "every shape here has bands short enough for the stationary kernel's sums"
            # ---- data gradient: the same kernel on the mirrored weight image
            L.check(lib.bp_conv_backward_data(C.byref(cv), C.byref(dyv), L.ptr(pb), L.ptr(wd), C.byref(dxv), L.IMPL_BF16,
                                              st), "backward_data")
            dx = from_view(dxb, CI, 0)
            e = G.rel_err(dx, dx_ref)
            print("backward_data ws=%d rel_err %.3e" % (ws_on, e))
            assert e < 4e-3, f"backward_data ws={ws_on}"
            assert outside_is_nan(dxb, CI, 0), "stores outside the view"
            res[ws_on] = (got, dx)
    finally:
        lib.bp_set_option(b"bf16_ws", -1)
    # the two kernels differ by accumulation order only: a bf16 ulp here and there
    assert G.rel_err(res[1][0], res[0][0]) < 8e-3 and G.rel_err(res[1][1], res[0][1]) < 8e-3
    assert np.mean(res[1][0] != res[0][0]) < 0.05 and np.mean(res[1][1] != res[0][1]) < 0.05
    # ... and the stationary kernel did run (otherwise the two results are bit-equal)
    assert not np.array_equal(res[1][0], res[0][0]), "the forward never reached the weights-stationary kernel"
    assert not np.array_equal(res[1][1], res[0][1]), "the data gradient never reached the weights-stationary kernel"


@pytest.mark.parametrize("h", [5, 9])
@pytest.mark.parametrize("act", ["none", "relu", "leaky"])
def test_strip_seam_is_exact(act, h):
    """Width 192 = three strips.  The input is zero except for the columns on each side of a strip boundary (63, 64,
    127, 128) and the two image edge columns (0, 191: neighbours in memory of the next / previous row, which a halo that
    forgot where the image ends would pick up).  Non-zero pixels hold 1, 2 or -4 in six of their channels; the weights are
    all 1/8; the pending activation is x -> x (scale 1, shift 0) with slope 1/4 for "leaky" and 0 for "relu".  Every
    product is a multiple of 1/8 and every partial sum an integer multiple of 1/8 below 6 pixels x 6 channels x 4 / 8 =
    18 in magnitude: exact in fp32 and in bf16 (8 significant bits cover integers to 256).  The output must EQUAL the
    float64 convolution."""
    lib = L.load()
    n, w = 2, 192
    rng = np.random.default_rng(100 + h)
    x = np.zeros((n, CI, h, w), np.float32)
    for col in (0, 63, 64, 127, 128, 191):
        for i in range(n):
            for y in range(h):
                ch = rng.choice(CI, 6, replace=False)
                x[i, ch, y, col] = rng.choice(np.array([1.0, 2.0, -4.0], np.float32), 6)
    wt = np.full((CO, CI, 3, 3), 0.125, np.float32)
    scale, shift = np.ones(CI, np.float32), np.zeros(CI, np.float32)
    slope = np.full(CI, {"none": 1.0, "relu": 0.0, "leaky": 0.25}[act], np.float32)
    xa = x.astype(np.float64) if act == "none" else np.where(x > 0, x, x * slope[0]).astype(np.float64)
    y_ref = ops.conv2d_fwd(xa, wt.astype(np.float64), 1, 1)
    assert np.abs(y_ref).max() <= 18.0 and np.array_equal(bf16_round(y_ref.astype(np.float32)).astype(np.float64), y_ref)
    assert np.abs(y_ref[..., 62:66]).max() > 0 and np.abs(y_ref[..., 126:130]).max() > 0
    cv = L.Conv(*CONV)
    st = G.stream()
    xb, xv = to_view(x, CI + 16, 8)
    keep, pw = G.pointwise(scale, shift, slope)
    wd = G.dev(wt)
    pf, pb = packed(lib, cv, wd, st)
    yb, yv = empty_view(n, h, w, CO, CO + 8, 8)
    assert lib.bp_conv_ws_kind(C.byref(cv), L.PACK_FWD, C.byref(xv), C.byref(yv)) == 3
    L.check(lib.bp_conv_forward(C.byref(cv), C.byref(xv), None if act == "none" else C.byref(pw), L.ptr(pf), L.ptr(wd),
                                None, C.byref(yv), L.IMPL_BF16, st), "forward")
    got = from_view(yb, CO, 8).astype(np.float64)
    bad = np.argwhere(got != y_ref)
    assert bad.size == 0, "first wrong (n, c, y, x): %s of %d, columns %s" % (bad[0], len(bad), sorted(set(bad[:, 3])))
    assert outside_is_nan(yb, CO, 8)


@pytest.mark.parametrize("col", [64, 63], ids=["first-column", "last-column"])
def test_strip_nan_crosses_the_seam(col):
    """One NaN at a strip's first (last) column reaches exactly the outputs whose 3 x 3 window covers it: those include
    the neighbouring strip's last (first) column, which sees it through its halo."""
    lib = L.load()
    n, h, w = 2, 6, 128
    rng = np.random.default_rng(7)
    x = bf16_round(rng.standard_normal((n, CI, h, w)).astype(np.float32))
    x[1, 37, 3, col] = np.nan
    wt = (rng.standard_normal((CO, CI, 3, 3)) * 0.05).astype(np.float32)
    keep, pw = G.pointwise(rng.uniform(0.5, 1.5, CI), rng.uniform(0.2, 0.6, CI), np.zeros(CI))
    cv = L.Conv(*CONV)
    st = G.stream()
    xb, xv = to_view(x, CI + 16, 8)
    wd = G.dev(wt)
    pf, pb = packed(lib, cv, wd, st)
    yb, yv = empty_view(n, h, w, CO, CO + 8, 8)
    assert lib.bp_conv_ws_kind(C.byref(cv), L.PACK_FWD, C.byref(xv), C.byref(yv)) == 3
    L.check(lib.bp_conv_forward(C.byref(cv), C.byref(xv), C.byref(pw), L.ptr(pf), L.ptr(wd), None, C.byref(yv),
                                L.IMPL_BF16, st), "forward")
    bad = np.isnan(from_view(yb, CO, 8))
    assert bad[1, :, 2:5, col - 1:col + 2].all() and bad.sum() == CO * 9
