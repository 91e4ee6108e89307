"""GPU: bp_unary_forward (kinds 0-3) and bp_unary_backward through the C ABI against the float64 forms of
tests/unary_ref.py, on views that take each of the kernels' paths:

  (2, 9, 13, 3), cstride 5, coff 2          one element per thread, ragged
  (3, 5, 7, 1) dense                        105 elements: the flat 16-byte path and its one-element tail
  (2, 16, 16, 8) at coff 8 of 16 channels   channel quads of a strided slice
  (2, 8, 8, 5) at coff 3 of 8 channels      must run one element per thread
  (2, 8, 8, 16) dense                       channel quads
  (8, 128, 128, 32) dense                   4.2 M elements: 4096 workgroups of the one-quad-per-thread grid

Planted in every input: +-0, |v| = 30, v = 20 and the next float32 above it (softplus' threshold), +-inf and NaN.  A
non-finite reference value must be met exactly; NaN must appear where the reference has it and nowhere else.
Destinations are poisoned with NaN and every channel outside a view must stay NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import gpu_util as G
import pointwise_ref as R
import unary_ref as UR

pytestmark = pytest.mark.gpu

NAN = float("nan")
U32 = R.U32
TINY = 2.0 ** -149          # one float32 denormal: results that underflow
VIEWS = [((2, 9, 13, 3), 5, 2), ((3, 5, 7, 1), 1, 0), ((2, 16, 16, 8), 16, 8), ((2, 8, 8, 5), 8, 3),
         ((2, 8, 8, 16), 16, 0), ((8, 128, 128, 32), 32, 0)]
VIEW_IDS = ["scalar-ragged", "flat-tail", "quads-slice", "scalar-slice", "quads", "many-blocks"]
KINDS = [0, 1, 2, 3]
KIND_IDS = ["identity", "tanh", "sigmoid", "softplus"]
PLANTED = np.array([0.0, -0.0, 30.0, -30.0, 20.0, np.nextafter(np.float32(20.0), np.float32(21.0)), np.inf, -np.inf,
                    np.nan], np.float32)


def upload(a, cstride, coff, dtype=torch.float32):
    """NHWC array -> (device buffer whose other channels hold NaN, bp_view)."""
    n, h, w, c = a.shape
    buf = torch.full((n, h, w, cstride), NAN, dtype=torch.float32, device="cuda")
    buf[..., coff:coff + c] = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    buf = buf.to(dtype)
    return buf, L.View(buf.data_ptr(), n, h, w, c, cstride, coff, L.BF16 if dtype == torch.bfloat16 else L.F32)


def blank(shape, cstride, coff, dtype=torch.float32):
    n, h, w, c = shape
    buf = torch.full((n, h, w, cstride), NAN, dtype=dtype, device="cuda")
    return buf, L.View(buf.data_ptr(), n, h, w, c, cstride, coff, L.BF16 if dtype == torch.bfloat16 else L.F32)


def down(buf, c, coff):
    return buf[..., coff:coff + c].to(torch.float32).cpu().numpy().astype(np.float64)


def untouched(buf, c, coff):
    b = buf.to(torch.float32)
    assert torch.isnan(b[..., :coff]).all() and torch.isnan(b[..., coff + c:]).all(), "store outside the view"


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def within(got, ref, tol, what):
    """Finite reference values within ``tol``; infinities and NaN exactly where the reference has them."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert (np.isnan(got) == np.isnan(ref)).all(), f"{what}: NaN where the reference has none, or none where it has"
    inf = np.isinf(ref)
    assert (got[inf] == ref[inf]).all(), f"{what}: an infinity of the reference is not met"
    err = np.abs(got[fin] - ref[fin])
    tol = np.broadcast_to(tol, ref.shape)[fin]
    bad = ~(err <= tol)
    if bad.any():
        i = np.flatnonzero(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} outside the limit; first: got {got[fin][i]!r} ref "
                             f"{ref[fin][i]!r} tol {tol[i]!r}")


def draw(rng, shape, scale=3.0):
    """Float32 values with the planted ones spread over pixels and channels (stride coprime to the sizes used)."""
    a = R.f32(rng.standard_normal(shape) * scale)
    flat = a.reshape(-1)
    pos = (np.arange(len(PLANTED)) * 11 + 3) % flat.size
    flat[pos] = PLANTED.astype(np.float64)
    return a


def pw_params(rng, c):
    scale = rng.uniform(0.5, 1.5, c).astype(np.float32)
    shift = rng.uniform(-0.4, 0.4, c).astype(np.float32)
    slope = rng.uniform(0.05, 0.3, c).astype(np.float32)
    return scale, shift, slope


@pytest.mark.parametrize("with_pw", [False, True], ids=["no-pw", "pw"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("view", VIEWS, ids=VIEW_IDS)
def test_unary_forward(view, kind, with_pw):
    """tanh / sigmoid: the limit tests/test_gpu_pointwise.py::test_unary_forward holds them to, 4 ulp32(ref) + 2 U32 |v|;
    softplus: the 4 ulp32 the log-likelihood test allows ``softplus_f`` (expf and log1pf, 2 ulp each) plus the same term;
    identity: exact.  v is the activated input as the kernel forms it (one fmaf, one product: tests/pointwise_ref.act
    rounds at the same two points), so the pointwise adds nothing to the limit."""
    lib, st = L.load(), G.stream()
    shape, cs, co = view
    c = shape[-1]
    rng = np.random.default_rng(100 * kind + c + with_pw)
    x = draw(rng, shape)
    xb, xv = upload(x, cs, co)
    ob, ov = blank(shape, cs, co)
    keep, pw, v = None, None, x
    if with_pw:
        sc, sf, sl = pw_params(rng, c)
        keep, pws = G.pointwise(sc, sf, sl)
        pw = C.byref(pws)
        with np.errstate(invalid="ignore", over="ignore"):
            v = R.act(x, sc, sf, sl)
    L.check(lib.bp_unary_forward(C.byref(xv), pw, kind, C.byref(ov), st), "unary_forward")
    ref = UR.forward(v, kind)
    got = down(ob, c, co)
    with np.errstate(invalid="ignore"):
        tol = 0.0 if kind == 0 else 4 * ulp32(np.where(np.isfinite(ref), ref, 0.0)) + \
            2 * U32 * np.abs(np.where(np.isfinite(v), v, 0.0)) + TINY
    within(got, ref, tol, f"unary forward kind {kind}")
    untouched(ob, c, co)
    if kind == 3 and not with_pw:
        g32 = got.astype(np.float32)
        assert (g32[x > 20] == x[x > 20].astype(np.float32)).all(), "softplus is the identity above the threshold"


@pytest.mark.parametrize("with_dout2", [False, True], ids=["dout", "dout+dout2"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("view", VIEWS, ids=VIEW_IDS)
def test_unary_backward(view, kind, with_dout2):
    """d_in = (dout + dout2) * f'(y) against the float64 expression on the DEVICE's own float32 y (the forward's output).
    With U = 2^-24 and g = |dout| + |dout2|, the float32 roundings of the kernel's expression are
      the sum dout + dout2 (1, none without dout2) and the final product (1), each U of the result, and
      tanh     y*y and 1 - y*y (or one fused rounding): U y^2 + U |1 - y^2|  -> |err| <= U g (3 |1 - y^2| + y^2)
               <= 4 U g (1 + y^2), the K of test_tanh_l1_backward;
      sigmoid  1 - y and y (1 - y): 2 U y (1 - y)                           -> |err| <= 4 U g y (1 - y) to first order;
               held to 4 U g |y| (1 + |y|), which covers the second order;
      softplus expm1f, a library call: 2 ulp of f'                          -> |err| <= 2 U g f' + 2 ulp32(f') g;
      identity nothing                                                      -> |err| <= U |dout + dout2|, 0 without dout2.
    A product that underflows may be off by one denormal."""
    lib, st = L.load(), G.stream()
    shape, cs, co = view
    c = shape[-1]
    rng = np.random.default_rng(1000 + 100 * kind + c + with_dout2)
    x = draw(rng, shape)
    xb, xv = upload(x, cs, co)
    yb, yv = blank(shape, cs, co)
    L.check(lib.bp_unary_forward(C.byref(xv), None, kind, C.byref(yv), st), "unary_forward")
    y = down(yb, c, co)
    d1 = draw(rng, shape, 1.0)
    d1b, d1v = upload(d1, cs, co)
    d2 = d2b = d2v = None
    if with_dout2:
        d2 = R.f32(rng.standard_normal(shape))
        # a second contribution is a dense buffer of its own (Slot.claim_grad) where the quad path can take it
        d2b, d2v = upload(d2, *((c, 0) if c % 4 == 0 or cs == c else (cs, co)))
    ob, ov = blank(shape, cs, co)
    L.check(lib.bp_unary_backward(C.byref(d1v), None if d2v is None else C.byref(d2v), C.byref(yv), kind, C.byref(ov),
                                  st), "unary_backward")
    ref = UR.backward(d1, d2, y, kind)
    got = down(ob, c, co)
    fin = lambda a: np.where(np.isfinite(a), a, 0.0)                                  # noqa: E731
    g = np.abs(fin(d1)) + (0.0 if d2 is None else np.abs(d2))
    yf = fin(y)
    if kind == 0:
        tol = U32 * g if with_dout2 else 0.0
    elif kind == 1:
        tol = 4 * U32 * g * (1 + yf * yf) + TINY
    elif kind == 2:
        tol = 4 * U32 * g * np.abs(yf) * (1 + np.abs(yf)) + TINY
    else:
        fp = fin(UR.derivative(yf, 3))
        tol = 2 * U32 * g * np.abs(fp) + 2 * ulp32(fp) * g + TINY
    within(got, ref, tol, f"unary backward kind {kind}")
    untouched(ob, c, co)


@pytest.mark.parametrize("kind", [1, 3], ids=["tanh", "softplus"])
def test_backward_in_place(kind):
    """d_in may be dout itself (every thread reads its elements before it writes them)."""
    lib, st = L.load(), G.stream()
    shape, cs, co = (2, 8, 8, 16), 16, 0
    rng = np.random.default_rng(7 + kind)
    y = R.f32(UR.forward(R.f32(rng.standard_normal(shape) * 2), kind))
    d = R.f32(rng.standard_normal(shape))
    yb, yv = upload(y, cs, co)
    ab, av = upload(d, cs, co)
    bb, bv = upload(d, cs, co)
    ob, ov = blank(shape, cs, co)
    L.check(lib.bp_unary_backward(C.byref(av), None, C.byref(yv), kind, C.byref(ov), st), "unary_backward")
    L.check(lib.bp_unary_backward(C.byref(bv), None, C.byref(yv), kind, C.byref(bv), st), "unary_backward in place")
    assert torch.equal(ob, bb)


def test_bf16_views_are_unsupported_and_nothing_is_written():
    lib, st = L.load(), G.stream()
    shape = (2, 8, 8, 8)
    rng = np.random.default_rng(5)
    x = R.f32(rng.standard_normal(shape))
    for kind in KINDS:
        for bf_in, bf_out in ((True, True), (True, False), (False, True)):
            xb, xv = upload(x, 8, 0, torch.bfloat16 if bf_in else torch.float32)
            ob, ov = blank(shape, 8, 0, torch.bfloat16 if bf_out else torch.float32)
            assert lib.bp_unary_forward(C.byref(xv), None, kind, C.byref(ov), st) == L.BP_EUNSUPPORTED
            for which in range(4):
                vs = [upload(x, 8, 0, torch.bfloat16 if which == i else torch.float32) for i in range(3)]
                db, dv = blank(shape, 8, 0, torch.bfloat16 if which == 3 else torch.float32)
                rc = lib.bp_unary_backward(C.byref(vs[0][1]), C.byref(vs[1][1]), C.byref(vs[2][1]), kind, C.byref(dv), st)
                assert rc == L.BP_EUNSUPPORTED
                torch.cuda.synchronize()
                assert torch.isnan(db.to(torch.float32)).all()
            torch.cuda.synchronize()
            assert torch.isnan(ob.to(torch.float32)).all()
    # views that are not one grid, and kinds outside 0..3, stay invalid arguments
    xb, xv = upload(x, 8, 0)
    ob, ov = blank((2, 8, 8, 4), 4, 0)
    assert lib.bp_unary_forward(C.byref(xv), None, 1, C.byref(ov), st) == L.BP_EINVAL
    ob, ov = blank(shape, 8, 0)
    assert lib.bp_unary_forward(C.byref(xv), None, 4, C.byref(ov), st) == L.BP_EINVAL
    assert lib.bp_unary_backward(C.byref(xv), None, C.byref(xv), -1, C.byref(ov), st) == L.BP_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(ob).all()


def test_vector_and_scalar_paths_give_the_same_bits():
    """The arithmetic per element does not depend on the path: a dense 8-channel tensor (channel quads) and the same
    values inside a 9-channel buffer at offset 1 (one element per thread), every kind, with a pending pointwise."""
    lib, st = L.load(), G.stream()
    shape = (2, 16, 16, 8)
    rng = np.random.default_rng(11)
    x = draw(rng, shape)
    sc, sf, sl = pw_params(rng, 8)
    keep, pws = G.pointwise(sc, sf, sl)
    d = R.f32(rng.standard_normal(shape))
    for kind in KINDS:
        outs = []
        for cs, co in ((8, 0), (9, 1)):
            xb, xv = upload(x, cs, co)
            ob, ov = blank(shape, cs, co)
            L.check(lib.bp_unary_forward(C.byref(xv), C.byref(pws), kind, C.byref(ov), st), "unary_forward")
            db, dv = upload(d, cs, co)
            gb, gv = blank(shape, cs, co)
            L.check(lib.bp_unary_backward(C.byref(dv), None, C.byref(ov), kind, C.byref(gv), st), "unary_backward")
            outs.append((ob[..., co:co + 8].contiguous(), gb[..., co:co + 8].contiguous()))
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), kind
