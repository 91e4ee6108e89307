"""GPU: the streaming, batch-norm, loss-head, paint and optimiser kernels (csrc/pointwise.hip, csrc/pointwise_bf16.hip,
csrc/paint.hip) through the C ABI, against the float64 references of tests/pointwise_ref.py.

Limits follow from the arithmetic each contract states:
  * double sums of terms that are exact in double (fp32 inputs: g, g*raw, d*t, x, x^2 are products of two float32s):
    the kernels add at most a few thousand terms in a row, so |err| <= 1e-12 * sum|term|;
  * bf16 paths add groups of <= 4 terms in fp32 before the double accumulators: |err| <= 2e-6 * sum|term|;
  * elementwise fp32 outputs: 2 float32 ulp of the float64 value plus the rounding of the formula's intermediate
    terms (the cancellation term, stated next to each check); transcendental fp32 library calls count 2 ulp each;
  * bf16 outputs: 1 bf16 ulp plus that same term;
  * loss statistics: 1e-6 of the sum of magnitudes behind them.
Destinations are poisoned with NaN and every channel outside a view is checked to stay NaN.  Pre-activations are
drawn with |t| >= 1e-3 (so the fp32 mask is unambiguous) except for planted exact zeros."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import gpu_util as G
import pointwise_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
U32, UBF = R.U32, R.UBF


# ------------------------------------------------------------------------------------------------------- helpers
def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def upload(a, bf16=False, cstride=None, coff=0):
    """NHWC array -> (device buffer whose other channels hold NaN, bp_view)."""
    n, h, w, c = a.shape
    cs = c if cstride is None else cstride
    buf = torch.full((n, h, w, cs), NAN, dtype=torch.float32, device="cuda")
    buf[..., coff:coff + c] = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    if bf16:
        buf = buf.to(torch.bfloat16)
    return buf, L.View(buf.data_ptr(), n, h, w, c, cs, coff, L.BF16 if bf16 else L.F32)


def blank(n, h, w, c, bf16=False, cstride=None, coff=0):
    cs = c if cstride is None else cstride
    buf = torch.full((n, h, w, cs), NAN, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    return buf, L.View(buf.data_ptr(), n, h, w, c, cs, coff, L.BF16 if bf16 else L.F32)


def down(buf, c, coff=0):
    return buf[..., coff:coff + c].to(torch.float32).cpu().numpy().astype(np.float64)


def untouched(buf, c, coff=0):
    """Nothing outside channels [coff, coff + c) was written."""
    b = buf.to(torch.float32)
    assert torch.isnan(b[..., :coff]).all() and torch.isnan(b[..., coff + c:]).all(), "store outside the view"


def host(t):
    return t.cpu().numpy().astype(np.float64)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def ulpbf(x):
    """bf16 ulp of |x| (8 significant bits)."""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, 2.0 ** (e - 7), 2.0 ** -133)


def within(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    if bad.any():
        i = np.flatnonzero(bad.ravel())[0]
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} outside the limit; first at flat {i}: got "
                             f"{got.ravel()[i]!r} ref {ref.ravel()[i]!r} tol {np.broadcast_to(tol, got.shape).ravel()[i]!r}")


def same_bits(a, b, what):
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    assert a.dtype == b.dtype and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8)), what


def workspace(nbytes):
    return torch.full((max(nbytes, 8) // 8 + 1,), NAN, dtype=torch.float64, device="cuda")


def pw_params(rng, c):
    scale = rng.uniform(0.5, 1.5, c).astype(np.float32)
    shift = rng.uniform(-0.4, 0.4, c).astype(np.float32)
    slope = rng.uniform(0.0, 0.3, c).astype(np.float32)
    shift[0] = 0.0                                       # channel 0: raw == 0 gives t == 0 exactly
    return scale, shift, slope


def draw_raw(rng, shape, scale, shift, bf16):
    """raw with |t| >= 1e-3 except for planted exact zeros of t (channel 0)."""
    rnd = bf16_round if bf16 else R.f32
    raw = rnd(rng.standard_normal(shape) * 1.3)
    raw[..., 0].flat[::7] = 0.0
    planted = np.zeros(shape, bool)
    planted[..., 0].flat[::7] = True
    for _ in range(20):
        t = R.pre_act(raw, scale, shift)
        bad = (np.abs(t) < 1e-3) & ~planted
        if not bad.any():
            return raw
        raw[bad] = rnd(raw[bad] + np.sign(raw[bad] + 1e-9) * 0.02 + 0.01)
    raise AssertionError("could not draw raw away from the mask edge")


# ------------------------------------------------------------------------------------------------- shapes
# fp32 channel counts: the fast path (dense, power of two <= 1024, aligned) and the scalar path (strided view, or a
# count the fast path does not take).  320 > 256: the scalar kernels take two passes; 2048 > 1024: scalar only.
F32_CASES = ([(c, "fast") for c in (1, 2, 4, 8, 128, 1024)] + [(c, "strided") for c in (1, 2, 4, 8, 128, 1024)] +
             [(c, "dense") for c in (5, 96, 320)] + [(2048, "dense")])
BF16_CHANNELS = (8, 16, 128, 1024)


def f32_shape(c, size):
    """'one': one block of either plan.  'multi': several blocks of both plans (> 256 pixels, > 2048 float4) with a
    partial last chunk."""
    if size == "one":
        npix = max(2, min(256, 4096 // c))
        return (1, 2, npix // 2)
    npix = max(300, (3 * 8192 + 1000) // c)
    w = 2 * math.ceil(npix / 28) + 1                     # odd width: a ragged last chunk
    return (2, 7, w + (w % 2 if c == 1 else 0))          # (c = 1: an element count divisible by 4)


def bf16_shape(c, size):
    """'one': one block; 'multi': three reduction blocks (the last partial) and, in the apply kernels, threads with
    an odd number of 16-byte units (the tail unit runs); 'odd': one block, fifteen or sixteen units per thread."""
    units = {"one": 256, "multi": 8692, "odd": 3940}[size]
    npix = max(1, units * 8 // c)
    return (1, 1, npix)


def view_args(path, c):
    return dict(cstride=c + 5, coff=3) if path == "strided" else {}


# ----------------------------------------------------------------------------------- the batch-norm backward chain
def _chain(c, shape, bf16, vargs, rng, variants):
    lib = L.load()
    st = G.stream()
    n, h, w = shape
    rnd = bf16_round if bf16 else R.f32
    scale, shift, slope = pw_params(rng, c)
    keep, pw = G.pointwise(scale, shift, slope)
    raw = draw_raw(rng, (n, h, w, c), scale, shift, bf16)
    dout = rnd(rng.standard_normal(raw.shape))
    dout2 = rnd(rng.standard_normal(raw.shape))
    skip = rng.standard_normal(raw.shape)
    aout = rnd(R.act(raw, scale, shift, slope) + skip)  # sign differs from t's where |skip| is large
    rb, rv = upload(raw, bf16, **vargs)
    db, dv = upload(dout, bf16, **vargs)
    d2b, d2v = upload(dout2, bf16, **vargs)
    ab, av = upload(aout, bf16, **vargs)
    ws_bytes = lib.bp_act_backward_workspace(C.byref(rv))
    assert ws_bytes > 0
    ws = workspace(ws_bytes)
    tol_sum = 2e-6 if bf16 else 1e-12

    # ---- channel sums (batch-norm statistics) and the finalize
    sums2 = torch.full((2 * c,), NAN, dtype=torch.float64, device="cuda")
    nbs = lib.bp_channel_sums_workspace(C.byref(rv))
    L.check(lib.bp_channel_sums(C.byref(rv), L.ptr(sums2), L.ptr(ws), nbs, st), "channel_sums")
    ref2 = R.channel_sums(raw)
    mag2 = np.stack([np.abs(raw).reshape(-1, c).sum(0), (raw * raw).reshape(-1, c).sum(0)])
    within(host(sums2).reshape(2, c), ref2, tol_sum * mag2 + 1e-300, "channel_sums")
    count = float(n * h * w)
    gam, bet = G.dev(rng.uniform(0.5, 1.5, c)), G.dev(rng.uniform(-0.2, 0.2, c))
    rm, rvar = G.dev(rng.standard_normal(c) * 0.1), G.dev(rng.uniform(0.5, 2.0, c))
    rm0, rv0 = host(rm), host(rvar)
    sc_o, sf_o = torch.full((c,), NAN, device="cuda"), torch.full((c,), NAN, device="cuda")
    mean = torch.full((c,), NAN, dtype=torch.float64, device="cuda")
    inv = torch.full((c,), NAN, dtype=torch.float64, device="cuda")
    L.check(lib.bp_bn_finalize(L.ptr(sums2), count, c, L.ptr(gam), L.ptr(bet), 1e-5, 0.1, L.ptr(rm), L.ptr(rvar),
                               None, L.ptr(sc_o), L.ptr(sf_o), L.ptr(mean), L.ptr(inv), st), "bn_finalize")
    fin = R.bn_finalize(host(sums2).reshape(2, c), count, host(gam), host(bet), 1e-5, 0.1, rm0, rv0)
    # (double arithmetic on the sums: the variance subtracts mean^2 -- cancellation term 4 ulp64 of (s1/n + mean^2))
    var_mag = host(sums2)[c:] / count + fin["mean"] ** 2
    var_eps = 1.0 / fin["invstd"] ** 2
    within(host(mean), fin["mean"], 4e-16 * np.abs(fin["mean"]), "bn_finalize mean")
    within(host(inv), fin["invstd"], fin["invstd"] * (4e-16 + 4e-16 * var_mag / var_eps), "bn_finalize invstd")
    within(host(sc_o), fin["scale"], 2 * ulp32(fin["scale"]) + 1e-12 * np.abs(fin["scale"]), "bn_finalize scale")
    within(host(sf_o), fin["shift"], 2 * ulp32(fin["shift"]) + 2 * U32 * np.abs(fin["mean"] * fin["scale"]),
           "bn_finalize shift")
    within(host(rm), fin["running_mean"], 2 * ulp32(fin["running_mean"]) + 2 * U32 * np.abs(fin["mean"]), "running_mean")
    within(host(rvar), fin["running_var"], 2 * ulp32(fin["running_var"]) + 1e-12, "running_var")

    # ---- activation backward: every (dout2, act_out, g written) variant
    sums3 = torch.full((3 * c,), NAN, dtype=torch.float64, device="cuda")
    for has_d2, has_ao, has_g in variants:
        ref_g, ref_s, mags = R.act_backward(dout, raw, scale, shift, slope, dout2 if has_d2 else None,
                                            aout if has_ao else None)
        gb, gv = blank(n, h, w, c, bf16, **vargs)
        sums3.fill_(NAN)
        args = (C.byref(dv), C.byref(d2v) if has_d2 else None, C.byref(rv), C.byref(pw), C.byref(av) if has_ao else None,
                C.byref(gv) if has_g else None, L.ptr(sums3), L.ptr(ws), ws_bytes, st)
        tag = f"act_backward d2={has_d2} ao={has_ao} g={has_g}"
        L.check(lib.bp_act_backward(*args), tag)
        within(host(sums3).reshape(3, c), ref_s, tol_sum * mags + 1e-300, tag + " sums")
        if has_g:
            # g is d or d*slope, one fp32 rounding (bf16: then one bf16 rounding) -- the reference rounds the same way
            assert np.array_equal(down(gb, c, vargs.get("coff", 0)), rnd(ref_g)), tag + " g"
            untouched(gb, c, vargs.get("coff", 0))
        else:
            assert torch.isnan(gb.to(torch.float32)).all(), tag + ": g = NULL must write nothing"
    # reproducible: a second identical call returns the same bits
    first = sums3.clone()
    L.check(lib.bp_act_backward(*args), "act_backward again")
    same_bits(sums3, first, "act_backward sums are not reproducible")

    # ---- bp_act_backward_bn == bp_act_backward + bp_bn_backward_finalize, bit for bit
    fin_out = lambda: [torch.full((c,), NAN, device="cuda"), torch.full((c,), NAN, device="cuda"),
                       torch.full((4 * c,), NAN, dtype=torch.float64, device="cuda")]
    dga, dbe, coef = fin_out()
    sA = torch.full((3 * c,), NAN, dtype=torch.float64, device="cuda")
    L.check(lib.bp_act_backward(C.byref(dv), C.byref(d2v), C.byref(rv), C.byref(pw), C.byref(av), None, L.ptr(sA),
                                L.ptr(ws), ws_bytes, st), "act_backward")
    L.check(lib.bp_bn_backward_finalize(L.ptr(sA), count, c, L.ptr(gam), L.ptr(mean), L.ptr(inv), 0.5, L.ptr(dga),
                                        L.ptr(dbe), L.ptr(coef), st), "bn_backward_finalize")
    dga2, dbe2, coef2 = fin_out()
    sB = torch.full((3 * c,), NAN, dtype=torch.float64, device="cuda")
    bf = L.BnBackwardFin(count, gam.data_ptr(), mean.data_ptr(), inv.data_ptr(), 0.5, dga2.data_ptr(), dbe2.data_ptr(),
                         coef2.data_ptr())
    L.check(lib.bp_act_backward_bn(C.byref(dv), C.byref(d2v), C.byref(rv), C.byref(pw), C.byref(av), None, L.ptr(sB),
                                   C.byref(bf), L.ptr(ws), ws_bytes, st), "act_backward_bn")
    for a, b, what in ((sA, sB, "sums"), (dga, dga2, "dgamma"), (dbe, dbe2, "dbeta"), (coef, coef2, "coefficients")):
        same_bits(b, a, "act_backward_bn " + what + " differ from act_backward + bn_backward_finalize")
    # the finalize against its float64 statement on the same sums
    s_h = host(sA).reshape(3, c)
    bw = R.bn_backward_finalize(s_h[:2], count, host(gam), host(mean), host(inv), pscale=0.5)
    canc = host(inv) * (np.abs(s_h[1]) + np.abs(host(mean) * s_h[0]))         # |inv| (|S1| + |mean S0|)
    within(host(dga), bw["dgamma"], 2 * ulp32(bw["dgamma"]) + 4e-16 * 0.5 * canc, "dgamma")
    within(host(dbe), bw["dbeta"], 2 * ulp32(bw["dbeta"]), "dbeta")
    cf = host(coef).reshape(4, c)
    within(cf[[0, 1, 3]], bw["coef"][[0, 1, 3]], 4e-16 * np.abs(bw["coef"][[0, 1, 3]]), "coefficients A, mg, mean")
    within(cf[2], bw["coef"][2], 8e-16 * np.abs(host(gam) * host(inv) ** 2) * canc / count, "coefficient B")

    # ---- batch-norm backward apply (g given), fresh and aliased to g
    g_ref, _, _ = R.act_backward(dout, raw, scale, shift, slope, dout2, aout)
    gq = rnd(g_ref)
    gb, gv = upload(gq, bf16, **vargs)
    ob, ov = blank(n, h, w, c, bf16, **vargs)
    L.check(lib.bp_bn_backward_apply(C.byref(gv), C.byref(rv), L.ptr(coef), C.byref(ov), st), "bn_backward_apply")
    A, Gm, B, M = cf
    ref = R.bn_apply(gq, raw, cf)
    K = np.abs(A) * (np.abs(gq) + np.abs(Gm)) + np.abs(B) * (np.abs(raw) + np.abs(M))
    tol_apply = (ulpbf(ref) + 8 * U32 * K) if bf16 else (2 * ulp32(ref) + 4e-16 * K)
    coff = vargs.get("coff", 0)
    within(down(ob, c, coff), ref, tol_apply, "bn_backward_apply")
    untouched(ob, c, coff)
    L.check(lib.bp_bn_backward_apply(C.byref(gv), C.byref(rv), L.ptr(coef), C.byref(gv), st), "bn_backward_apply alias")
    same_bits(gb, ob, "bn_backward_apply with out aliasing g")

    # ---- activation + batch-norm backward apply (g recomputed), every (dout2, act_out) variant, fresh and aliased
    for has_d2, has_ao in ((0, 0), (0, 1), (1, 0), (1, 1)):
        g_ref, _, _ = R.act_backward(dout, raw, scale, shift, slope, dout2 if has_d2 else None, aout if has_ao else None)
        ref = R.bn_apply(g_ref, raw, cf)
        K = np.abs(A) * (np.abs(g_ref) + np.abs(Gm)) + np.abs(B) * (np.abs(raw) + np.abs(M))
        tol = (ulpbf(ref) + 8 * U32 * K) if bf16 else (2 * ulp32(ref) + 4e-16 * K)
        ob, ov = blank(n, h, w, c, bf16, **vargs)
        tag = f"act_bn_backward_apply d2={has_d2} ao={has_ao}"
        L.check(lib.bp_act_bn_backward_apply(C.byref(dv), C.byref(d2v) if has_d2 else None, C.byref(rv), C.byref(pw),
                                             C.byref(av) if has_ao else None, L.ptr(coef), C.byref(ov), st), tag)
        within(down(ob, c, coff), ref, tol, tag)
        untouched(ob, c, coff)
        cb, cv = upload(dout, bf16, **vargs)
        L.check(lib.bp_act_bn_backward_apply(C.byref(cv), C.byref(d2v) if has_d2 else None, C.byref(rv), C.byref(pw),
                                             C.byref(av) if has_ao else None, L.ptr(coef), C.byref(cv), st), tag)
        same_bits(cb, ob, tag + " with out aliasing dout")

    # ---- residual tail
    ksc, ksf, ksl = pw_params(rng, c)
    keep2, kpw = G.pointwise(ksc, ksf, ksl)
    skipv = rnd(rng.standard_normal(raw.shape))
    sb, sv = upload(skipv, bf16, **vargs)
    ob, ov = blank(n, h, w, c, bf16, **vargs)
    L.check(lib.bp_residual_forward(C.byref(rv), C.byref(pw), C.byref(sv), C.byref(kpw), 0.2, C.byref(ov), st),
            "residual_forward")
    t = R.pre_act(raw, scale, shift)
    u = R.act(skipv, ksc, ksf, ksl)
    ref = R.residual_forward(raw, scale, shift, skipv, ksc, ksf, ksl, 0.2, f32_round=False)
    K = 2 * U32 * (np.abs(t) + np.abs(u))                # (the fp32 sum t + act(skip) and its inputs' roundings)
    within(down(ob, c, coff), ref, (ulpbf(ref) if bf16 else 2 * ulp32(ref)) + K, "residual_forward")
    untouched(ob, c, coff)


ALL8 = [(d2, ao, g) for d2 in (0, 1) for ao in (0, 1) for g in (0, 1)]


@pytest.mark.parametrize("size", ["one", "multi"])
@pytest.mark.parametrize("c,path", F32_CASES, ids=lambda v: str(v))
def test_f32_batchnorm_chain(c, path, size):
    rng = np.random.default_rng(c * 7 + len(path) + len(size))
    _chain(c, f32_shape(c, size), False, view_args(path, c), rng, ALL8)


@pytest.mark.parametrize("size", ["one", "multi", "odd"])
@pytest.mark.parametrize("c", BF16_CHANNELS)
def test_bf16_batchnorm_chain(c, size):
    rng = np.random.default_rng(c * 5 + len(size))
    _chain(c, bf16_shape(c, size), True, {}, rng, ALL8)


@pytest.mark.parametrize("shape,vargs", [((1, 1040, 1024, 16), {}),                      # fast_plan: > 2048 blocks;
                                          ((1, 521, 513, 1), dict(cstride=2, coff=1))],  # apply grid > 4096 blocks
                         ids=["fast-cap", "scalar-cap"])                                 # scalar: > 1024 blocks
def test_f32_reduction_caps(shape, vargs):
    """One case past each block cap (more than 16 777 216 elements on the fast path; more than 262 144 pixels on the
    scalar path): channel sums, activation backward and both apply kernels."""
    lib = L.load()
    st = G.stream()
    rng = np.random.default_rng(99)
    n, h, w, c = shape
    scale, shift, slope = pw_params(rng, c)
    keep, pw = G.pointwise(scale, shift, slope)
    raw = draw_raw(rng, shape, scale, shift, False)
    dout = R.f32(rng.standard_normal(shape))
    rb, rv = upload(raw, **vargs)
    db, dv = upload(dout, **vargs)
    ws_bytes = lib.bp_act_backward_workspace(C.byref(rv))
    ws = workspace(ws_bytes)
    s2 = torch.full((2 * c,), NAN, dtype=torch.float64, device="cuda")
    L.check(lib.bp_channel_sums(C.byref(rv), L.ptr(s2), L.ptr(ws), ws_bytes, st))
    mag = np.stack([np.abs(raw).reshape(-1, c).sum(0), (raw * raw).reshape(-1, c).sum(0)])
    within(host(s2).reshape(2, c), R.channel_sums(raw), 1e-12 * mag, "channel_sums")
    del mag
    gb, gv = blank(n, h, w, c, **vargs)
    s3 = torch.full((3 * c,), NAN, dtype=torch.float64, device="cuda")
    L.check(lib.bp_act_backward(C.byref(dv), None, C.byref(rv), C.byref(pw), None, C.byref(gv), L.ptr(s3), L.ptr(ws),
                                ws_bytes, st))
    g_ref, s_ref, mags = R.act_backward(dout, raw, scale, shift, slope)
    within(host(s3).reshape(3, c), s_ref, 1e-12 * mags, "act_backward sums")
    coff = vargs.get("coff", 0)
    assert np.array_equal(down(gb, c, coff), g_ref), "act_backward g"
    untouched(gb, c, coff)
    coef_h = np.stack([rng.uniform(0.5, 1.5, c), rng.standard_normal(c) * 0.01, rng.uniform(-0.1, 0.1, c),
                       rng.standard_normal(c) * 0.1])
    coef = G.dev(coef_h.ravel(), torch.float64)
    ob, ov = blank(n, h, w, c, **vargs)
    L.check(lib.bp_bn_backward_apply(C.byref(gv), C.byref(rv), L.ptr(coef), C.byref(ov), st))
    A, Gm, B, M = coef_h
    ref = R.bn_apply(g_ref, raw, coef_h)
    K = np.abs(A) * (np.abs(g_ref) + np.abs(Gm)) + np.abs(B) * (np.abs(raw) + np.abs(M))
    within(down(ob, c, coff), ref, 2 * ulp32(ref) + 4e-16 * K, "bn_backward_apply")
    untouched(ob, c, coff)
    ob2, ov2 = blank(n, h, w, c, **vargs)
    L.check(lib.bp_act_bn_backward_apply(C.byref(dv), None, C.byref(rv), C.byref(pw), None, L.ptr(coef), C.byref(ov2),
                                         st))
    same_bits(ob2, ob, "act_bn_backward_apply != bn_backward_apply of the same g")


@pytest.mark.parametrize("path", ["fast", "strided", "bf16"])
def test_nan_stays_in_its_channel(path):
    """A NaN in dout (channel 1) or raw (channel 2) reaches that channel's g and sums, and no other channel's."""
    lib = L.load()
    st = G.stream()
    rng = np.random.default_rng(7)
    c, bf16 = 8, path == "bf16"
    vargs = view_args(path, c)
    shape = (2, 9, 130, c)
    scale, shift, slope = pw_params(rng, c)
    keep, pw = G.pointwise(scale, shift, slope)
    raw = draw_raw(rng, shape, scale, shift, bf16)
    dout = (bf16_round if bf16 else R.f32)(rng.standard_normal(shape))
    dout[1, 4, 77, 1] = NAN
    raw[0, 8, 3, 2] = NAN
    rb, rv = upload(raw, bf16, **vargs)
    db, dv = upload(dout, bf16, **vargs)
    gb, gv = blank(*shape[:3], c, bf16, **vargs)
    ws_bytes = lib.bp_act_backward_workspace(C.byref(rv))
    ws = workspace(ws_bytes)
    s3 = torch.full((3 * c,), NAN, dtype=torch.float64, device="cuda")
    L.check(lib.bp_act_backward(C.byref(dv), None, C.byref(rv), C.byref(pw), None, C.byref(gv), L.ptr(s3), L.ptr(ws),
                                ws_bytes, st))
    s = host(s3).reshape(3, c)
    g = down(gb, c, vargs.get("coff", 0))
    assert np.isnan(g[1, 4, 77, 1]) and np.isnan(g).sum() == 1         # (a NaN t takes the negative branch: g finite)
    assert np.isnan(s[0, 1]) and np.isnan(s[1, 1]), "a NaN in dout must reach its channel's sums"
    assert np.isnan(s[1, 2]) and np.isnan(s[2, 2]), "a NaN in raw must reach its channel's sums"
    clean = [ch for ch in range(c) if ch not in (1, 2)]
    _, s_ref, mags = R.act_backward(dout, raw, scale, shift, slope)
    tol = (2e-6 if bf16 else 1e-12) * mags[:, clean]
    within(s[:, clean], s_ref[:, clean], tol, "sums of the clean channels")


def test_bf16_views_without_a_bf16_form_are_refused():
    lib = L.load()
    st = G.stream()
    ws = workspace(1 << 20)
    coef = torch.zeros(4 * 16, dtype=torch.float64, device="cuda")
    s = torch.zeros(3 * 16, dtype=torch.float64, device="cuda")
    for c, vargs in ((4, {}), (12, {}), (16, dict(cstride=24, coff=8))):
        xb, xv = upload(np.ones((1, 4, 8, c)), True, **vargs)
        ob, ov = blank(1, 4, 8, c, True, **vargs)
        rcs = [lib.bp_channel_sums(C.byref(xv), L.ptr(s), L.ptr(ws), 1 << 20, st),
               lib.bp_act_backward(C.byref(xv), None, C.byref(xv), None, None, C.byref(ov), L.ptr(s), L.ptr(ws), 1 << 20,
                                   st),
               lib.bp_bn_backward_apply(C.byref(xv), C.byref(xv), L.ptr(coef), C.byref(ov), st),
               lib.bp_act_bn_backward_apply(C.byref(xv), None, C.byref(xv), None, None, L.ptr(coef), C.byref(ov), st),
               lib.bp_residual_forward(C.byref(xv), None, C.byref(xv), None, 0.1, C.byref(ov), st)]
        assert rcs == [L.BP_EUNSUPPORTED] * 5, (c, vargs, rcs)
        assert lib.bp_channel_sums_workspace(C.byref(xv)) == 0 and lib.bp_act_backward_workspace(C.byref(xv)) == 0
        assert torch.isnan(ob.to(torch.float32)).all()


# -------------------------------------------------------------------------------------------------- loss heads
@pytest.mark.parametrize("predict_var,alpha", [(0, 1.0), (1, 0.3), (1, 1.0)], ids=["fixed", "a0.3", "a1"])
@pytest.mark.parametrize("hw", [(8, 16), (9, 13)], ids=["pow2", "ragged"])
@pytest.mark.parametrize("L_,c", [(1, 1), (2, 1), (1, 2), (2, 2)], ids=["L1c1", "L2c1", "L1c2", "L2c2"])
def test_loglik_head(L_, c, hw, predict_var, alpha):
    lib = L.load()
    st = G.stream()
    h, w = hw
    M = 3
    rng = np.random.default_rng(L_ * 10 + c + h + predict_var)
    softplus = int(not (L_ == 2 and c == 2))           # one case without the softplus
    x = R.f32(rng.standard_normal((M, c, h, w)))
    mu = R.f32(rng.standard_normal((L_ * M, h, w, c)) * 2)
    mu[0, 0, 0, :] = 23.5                              # above the softplus threshold of 20
    var = R.f32(rng.standard_normal((L_ * M, h, w, c)) * 0.5)
    # one head buffer, mean at channels [1, 1 + c), log-variance at [1 + c, 1 + 2c)
    head = np.concatenate([mu, var], axis=-1)
    hb, hv = upload(head, cstride=2 * c + 3, coff=1)
    mv = L.View(hb.data_ptr(), L_ * M, h, w, c, 2 * c + 3, 1, L.F32)
    vv = L.View(hb.data_ptr(), L_ * M, h, w, c, 2 * c + 3, 1 + c, L.F32)
    alpha, beta, lsc = (float(np.float32(v)) for v in (alpha, 0.7, 1.3))     # the struct's float fields
    ll = L.Loglik(M, L_, c, h, w, softplus, predict_var, alpha, beta, lsc)
    xd = G.dev(x)
    kl = torch.tensor([5.25], dtype=torch.float64, device="cuda")
    xmu = torch.full((L_ * M, c, h, w), NAN, device="cuda")
    xlv = torch.full((L_ * M, c, h, w), NAN, device="cuda")
    stats = torch.full((2 + 3 * c + 1,), NAN, device="cuda")
    nb = lib.bp_loglik_workspace(C.byref(ll))
    ws = workspace(nb)
    L.check(lib.bp_loglik_forward(C.byref(ll), L.ptr(xd), C.byref(mv), C.byref(vv), L.ptr(kl), L.ptr(xmu), L.ptr(xlv),
                                  L.ptr(stats), L.ptr(ws), nb, st), "loglik_forward")
    xm_ref, lv_ref, st_ref = R.loglik_forward(x, mu, var, 5.25, L_, softplus, predict_var, alpha, beta, lsc)
    # x_mu: torch's softplus in fp32 (expf then log1pf: 2 ulp each) or a copy
    within(host(xmu), xm_ref, 4 * ulp32(xm_ref) if softplus else 0.0, "x_mu")
    if predict_var:
        assert np.array_equal(host(xlv), lv_ref), "x_log_var"
    else:
        assert torch.isnan(xlv).all()
    # statistics: each term is a few fp32 operations on d = x - x_mu (rounding U32 (|x| + 5 |x_mu|))
    xr = np.tile(x, (L_, 1, 1, 1))
    d = xr - xm_ref
    dd = U32 * (np.abs(xr) + 5 * np.abs(xm_ref))
    mag_f = (0.5 * d * d + np.abs(d) * dd).sum(axis=(0, 2, 3)) / (M * L_) + 0.92
    mag_v = mag_f if not predict_var else ((0.5 * np.abs(lv_ref) + 0.5 * d * d / np.exp(lv_ref)
                                            + np.abs(d) * dd / np.exp(lv_ref)).sum(axis=(0, 2, 3)) / (M * L_) + 0.92)
    mag_l = (1 - alpha) * mag_f + alpha * mag_v if predict_var else mag_f
    got = host(stats)[:2 + 3 * c]
    within(got[2:2 + c], st_ref[2:2 + c], 1e-6 * mag_l, "log_likelihood")
    within(got[2 + c:2 + 2 * c], st_ref[2 + c:2 + 2 * c], 1e-6 * mag_f, "fixed_var")
    within(got[2 + 2 * c:], st_ref[2 + 2 * c:], 1e-6 * mag_v if predict_var else 0.0, "free_var")
    within(got[1], st_ref[1], 2 * ulp32(st_ref[1]), "KL_term")
    within(got[0], st_ref[0], 1e-6 * (lsc * mag_l.sum() + beta * abs(st_ref[1])), "ELBO")
    assert np.isnan(host(stats)[-1]), "stats written past 2 + 3c"

    # backward
    seed = torch.tensor([-1.5], device="cuda")
    gb = torch.full((L_ * M, h, w, 2 * c + 4), NAN, device="cuda")
    dmv = L.View(gb.data_ptr(), L_ * M, h, w, c, 2 * c + 4, 2, L.F32)
    dvv = L.View(gb.data_ptr(), L_ * M, h, w, c, 2 * c + 4, 2 + c, L.F32)
    L.check(lib.bp_loglik_backward(C.byref(ll), L.ptr(xd), C.byref(mv), C.byref(vv), L.ptr(seed), C.byref(dmv),
                                   C.byref(dvv), st), "loglik_backward")
    dmu_ref, dvar_ref = R.loglik_backward(x, mu, var, L_, -1.5, softplus, predict_var, alpha, lsc)
    s = 1.5 * lsc / (M * L_)
    dn = d.transpose(0, 2, 3, 1)
    ddn = dd.transpose(0, 2, 3, 1)
    if predict_var:
        xv = np.exp(var)
        fac = (1 - alpha) + alpha / xv
        within(down(gb, c, 2), dmu_ref, 8 * U32 * (np.abs(dmu_ref) + s * fac * np.abs(dn)) + s * fac * ddn, "d mu")
        K2 = s * alpha * (0.5 + 0.5 * dn * dn / xv)
        within(down(gb, c, 2 + c), dvar_ref, 8 * U32 * K2 + s * alpha * np.abs(dn) * ddn / xv, "d log var")
    else:
        within(down(gb, c, 2), dmu_ref, 8 * U32 * (np.abs(dmu_ref) + s * np.abs(dn)) + s * ddn, "d mu")
        assert torch.isnan(gb[..., 2 + c:2 + 2 * c]).all(), "d var written without predict_var"
    assert torch.isnan(gb[..., :2]).all() and torch.isnan(gb[..., 2 + 2 * c:]).all(), "store outside the views"


@pytest.mark.parametrize("prior", [False, True], ids=["std-prior", "prior-net"])
@pytest.mark.parametrize("L_,dims", [(1, (2, 3, 5, 7)), (2, (2, 3, 5, 7)), (2, (2, 4, 96, 96))],
                         ids=["L1", "L2", "L2-past-grid-cap"])
def test_latent_heads(L_, dims, prior):
    lib = L.load()
    st = G.stream()
    n, zc, zh, zw = dims
    rng = np.random.default_rng(L_ + zh + prior)
    c2 = 2 * zc
    q = R.f32(rng.standard_normal((n, zh, zw, c2)))
    p = R.f32(rng.standard_normal((n, zh, zw, c2)))
    sc, sf, sl = (rng.uniform(0.3, 0.8, c2).astype(np.float32), rng.uniform(-.2, .2, c2).astype(np.float32),
                  rng.uniform(0.05, 0.3, c2).astype(np.float32))
    keep, pw = G.pointwise(sc, sf, sl)
    qb, qv = upload(q, cstride=c2 + 3, coff=2)
    pb, pv = upload(p, cstride=c2 + 1, coff=1)
    eps = R.f32(rng.standard_normal((L_, n, zc, zh, zw)))
    ed = G.dev(eps)
    zb, zv = blank(L_ * n, zh, zw, zc, cstride=zc + 2, coff=1)
    nelem = n * zc * zh * zw
    stats = torch.full((4 * nelem + 1,), NAN, device="cuda")
    kl = torch.full((1,), NAN, dtype=torch.float64, device="cuda")
    lt = L.Latent(n, L_, zc, zh, zw, 1e-3)
    nblk = min(256, -(-nelem // 256))
    ws = workspace(nblk * 8)
    L.check(lib.bp_latent_forward(C.byref(lt), C.byref(qv), C.byref(pw), C.byref(pv) if prior else None,
                                  C.byref(pw) if prior else None, L.ptr(ed), L.ptr(stats), C.byref(zv), L.ptr(kl),
                                  L.ptr(ws), nblk * 8, st), "latent_forward")
    qa = R.act(q, sc, sf, sl)
    pa = R.act(p, sc, sf, sl) if prior else None
    s4_ref, z_ref, kl_ref = R.latent_forward(qa, eps, L_, 1e-3, pa)
    s4 = host(stats)
    assert np.isnan(s4[-1]), "stats4 written past its end"
    assert np.array_equal(s4[:-1].reshape(s4_ref.shape), s4_ref), "stats4 (the activated heads, copied)"
    lv = s4_ref[1]
    sd = np.exp(lv / 2) + 1e-3
    e = eps
    # z = fmaf(eps, expf(lv / 2) + min_z_var, mu): expf 2 ulp, the add and the fma one rounding each
    tol = 2 * ulp32(z_ref) + (4 * U32 * np.abs(e) * sd).reshape(L_ * n, zc, zh, zw).transpose(0, 2, 3, 1)
    within(down(zb, zc, 1), z_ref, tol, "z")
    untouched(zb, zc, 1)
    mu, _, pm, plv = s4_ref
    mags = np.sum((pm - mu) ** 2 / np.exp(plv) + np.exp(lv) / np.exp(plv) + np.abs(plv) + np.abs(lv) + 1)
    within(host(kl)[0], kl_ref, 1e-6 * mags, "kl_sum")                 # ~8 fp32 operations per term

    dz = R.f32(rng.standard_normal((L_ * n, zh, zw, zc)))
    dzb, dzv = upload(dz, cstride=zc + 1, coff=1)
    seed = torch.tensor([-1.0], device="cuda")
    dqb, dqv = blank(n, zh, zw, c2, cstride=c2 + 2, coff=2)
    dpb, dpv = blank(n, zh, zw, c2, cstride=c2 + 1, coff=0)
    L.check(lib.bp_latent_backward(C.byref(lt), C.byref(dzv), L.ptr(stats), L.ptr(ed), L.ptr(seed), 0.8, C.byref(dqv),
                                   C.byref(dpv) if prior else None, st), "latent_backward")
    dq_ref, dp_ref = R.latent_backward(dz, s4_ref, eps, L_, -1.0, 0.8)
    k = 0.8 * 0.5 / n
    dzn = dz.transpose(0, 3, 1, 2).reshape(L_, n, zc, zh, zw)
    pv_ = np.exp(plv)
    m_mu = np.abs(dzn).sum(0) + k * 2 * np.abs(pm - mu) / pv_
    m_lv = np.abs(dzn * e).sum(0) * 0.5 * np.exp(lv / 2) + k * (np.exp(lv) / pv_ + 1)
    nh = lambda a, b: np.concatenate([a, b], axis=1).transpose(0, 2, 3, 1)
    within(down(dqb, c2, 2), dq_ref, 8 * U32 * nh(m_mu, m_lv), "d q")
    untouched(dqb, c2, 2)
    if prior:
        m_p = nh(k * 2 * np.abs(pm - mu) / pv_, k * ((pm - mu) ** 2 / pv_ + np.exp(lv) / pv_ + 1))
        within(down(dpb, c2, 0), dp_ref, 8 * U32 * m_p, "d p")
        untouched(dpb, c2, 0)
    else:
        assert torch.isnan(dpb).all()


@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("c", [1, 2])
def test_bce_on_logits(c, target):
    lib = L.load()
    st = G.stream()
    rng = np.random.default_rng(int(target) + 3 * c)
    x = R.f32(rng.standard_normal((5, 9, 13, c)) * 6)
    x[1, 0, 0, 0], x[2, 1, 1, c - 1], x[3, 2, 2, 0] = 27.0, -26.0, 20.5
    xb, xv = upload(x, cstride=c + 3, coff=1)
    s = torch.full((1,), NAN, dtype=torch.float64, device="cuda")
    ws = workspace(256 * 8)
    L.check(lib.bp_bce_logits(C.byref(xv), 1, 4, target, L.ptr(s), L.ptr(ws), 256 * 8, st), "bce_logits")
    ref, mag = R.bce_logits(x, 1, 4, target)
    within(host(s)[0], ref, 4 * U32 * mag + 1e-300, "bce sum")            # log1pf(expf(z)): 2 + 2 ulp per term
    db, dv = blank(5, 9, 13, c, cstride=c + 2, coff=2)
    L.check(lib.bp_bce_logits_grad(C.byref(xv), 1, 4, target, 0.25, C.byref(dv), st), "bce_logits_grad")
    g = down(db, c, 2)
    gref = R.bce_logits_grad(x, 1, 4, target, 0.25)
    within(g[1:4], gref, 4 * U32 * 0.25 * (R.ops.sigmoid(x[1:4]) + target) + 1e-300, "bce grad")
    assert np.isnan(g[[0, 4]]).all(), "samples outside [n0, n1) written"
    untouched(db, c, 2)


@pytest.mark.parametrize("with_dfake", [True, False], ids=["d_fake", "no-d_fake"])
def test_l1_and_tanh_backward(with_dfake):
    lib = L.load()
    st = G.stream()
    rng = np.random.default_rng(31)
    n, h, w, c = 3, 9, 13, 2
    fake = R.f32(np.tanh(rng.standard_normal((n, h, w, c))))
    x = R.f32(rng.standard_normal((n, c, h, w)))
    x.transpose(0, 2, 3, 1)[0, 0, :5, :] = fake[0, 0, :5, :]            # diff == 0 exactly
    fb, fv = upload(fake, cstride=c + 2, coff=1)
    xd = G.dev(x)
    s = torch.full((1,), NAN, dtype=torch.float64, device="cuda")
    ws = workspace(256 * 8)
    L.check(lib.bp_l1_sum(C.byref(fv), L.ptr(xd), L.ptr(s), L.ptr(ws), 256 * 8, st), "l1_sum")
    mag = R.l1_sum(fake, x)
    within(host(s)[0], mag, 1e-12 * mag, "l1 sum")                       # |f - x| exact in double
    dfake = R.f32(rng.standard_normal(fake.shape)) if with_dfake else None
    if with_dfake:
        dfb, dfv = upload(dfake, cstride=c + 1, coff=0)
    db, dv = blank(n, h, w, c, cstride=c + 3, coff=3)
    L.check(lib.bp_tanh_l1_backward(C.byref(fv), L.ptr(xd), C.byref(dfv) if with_dfake else None, 0.6, C.byref(dv),
                                    st), "tanh_l1_backward")
    ref = R.tanh_l1_backward(fake, x, dfake, 0.6)
    K = ((np.abs(dfake) if with_dfake else 0) + 0.6) * (1 + fake * fake)
    got = down(db, c, 3)
    within(got, ref, 4 * U32 * K, "tanh_l1_backward")
    if not with_dfake:
        assert (got[0, 0, :5, :] == 0).all(), "sign(0) must be 0"
    untouched(db, c, 3)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["identity", "tanh", "sigmoid"])
def test_unary_forward(kind):
    lib = L.load()
    st = G.stream()
    rng = np.random.default_rng(41 + kind)
    n, h, w, c = 2, 9, 13, 3
    x = R.f32(rng.standard_normal((n, h, w, c)) * 3)
    sc, sf, sl = pw_params(rng, c)
    keep, pw = G.pointwise(sc, sf, sl)
    xb, xv = upload(x, cstride=c + 2, coff=2)
    ob, ov = blank(n, h, w, c, cstride=c + 1, coff=0)
    L.check(lib.bp_unary_forward(C.byref(xv), C.byref(pw), kind, C.byref(ov), st), "unary_forward")
    v = R.act(x, sc, sf, sl)
    ref = R.unary(v, kind)
    within(down(ob, c, 0), ref, 0.0 if kind == 0 else 4 * ulp32(ref) + 2 * U32 * np.abs(v), "unary")
    untouched(ob, c, 0)


# --------------------------------------------------------------------------------------------------------- paint
@pytest.mark.parametrize("hw", [(16, 16), (9, 13)], ids=["pow2", "ragged"])
@pytest.mark.parametrize("c,caux", [(1, 0), (1, 1), (2, 1)])
def test_paint_load_and_load2(c, caux, hw):
    lib = L.load()
    st = G.stream()
    h, w = hw
    n = 3
    rng = np.random.default_rng(c * 3 + caux + h)
    raw = R.f32(rng.uniform(0.0, 50.0, (n, c, h, w)))
    sk = np.stack([rng.uniform(1, 3, n), rng.uniform(2, 5, n)], axis=1)
    aux = R.f32(rng.uniform(0, 2, (n, caux))) if caux else None
    rd, skd = G.dev(raw), G.dev(sk, torch.float64)
    ad = G.dev(aux) if caux else None
    ct = c + caux
    ref = R.paint_load(raw, sk, aux)
    tol = ulp32(ref)                                    # a double log, one rounding to float32
    ob, ov = blank(n, h, w, ct, cstride=ct + 2, coff=1)
    L.check(lib.bp_paint_load(L.ptr(rd), c, L.ptr(skd), L.ptr(ad), caux, C.byref(ov), st), "paint_load")
    within(down(ob, ct, 1), ref, tol, "paint_load")
    untouched(ob, ct, 1)
    ob1, ov1 = blank(n, h, w, ct, cstride=ct + 3, coff=3)
    ob2, ov2 = blank(n, h, w, ct, cstride=ct + 1, coff=0)
    L.check(lib.bp_paint_load2(L.ptr(rd), c, L.ptr(skd), L.ptr(ad), caux, C.byref(ov1), C.byref(ov2), st), "load2")
    assert np.array_equal(down(ob1, ct, 3), down(ob, ct, 1)) and np.array_equal(down(ob2, ct, 0), down(ob, ct, 1))
    untouched(ob1, ct, 3)
    untouched(ob2, ct, 0)


@pytest.mark.parametrize("hw", [(16, 16), (9, 13)], ids=["pow2", "ragged"])
@pytest.mark.parametrize("c,softplus", [(1, 0), (1, 1), (2, 1), (3, 0)])
def test_paint_store(c, softplus, hw):
    lib = L.load()
    st = G.stream()
    h, w = hw
    n = 3
    rng = np.random.default_rng(c * 5 + softplus + h)
    src = R.f32(rng.standard_normal((n, h, w, c)) * 1.5)
    src[0, 0, 0, 0] = 30.0                              # softplus above its threshold
    sc, sf, sl = pw_params(rng, c)
    keep, pw = G.pointwise(sc, sf, sl)
    ks = np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(1, 4, n)], axis=1)
    ks[0, 0] = 0.25
    sb, sv = upload(src, cstride=c + 3, coff=2)
    kd = G.dev(ks, torch.float64)
    dst = torch.full((n, c, h, w), NAN, device="cuda")
    L.check(lib.bp_paint_store(C.byref(sv), C.byref(pw), softplus, L.ptr(kd), L.ptr(dst), st), "paint_store")
    v = R.act(src, sc, sf, sl)
    ref = R.paint_store(v, ks, softplus=bool(softplus))
    vs = R.ops.softplus(v) if softplus else v
    t = (vs * ks[:, 0, None, None, None]).transpose(0, 3, 1, 2)
    e = np.exp(t)
    sig = ks[:, 1, None, None, None]
    dv = 4 * U32 if softplus else 0.0                   # softplus in fp32: expf + log1pf
    # t = v * (float) k: two roundings; (float) exp(t): one; e - 1 in fp32: one; the double product: one
    tol = sig * (e * np.abs(t) * (dv + 2 * U32) + 2 * U32 * e) + 2 * ulp32(ref)
    within(host(dst), ref, tol, "paint_store")


# ---------------------------------------------------------------------------------------------- Adam, glue, caps
def test_adam_step_and_device_scalars():
    lib = L.load()
    st = G.stream()
    rng = np.random.default_rng(51)
    n = 1037
    p0, g = R.f32(rng.standard_normal(n)), R.f32(rng.standard_normal(n) * 0.1)
    m0, v0 = R.f32(rng.standard_normal(n) * 0.01), R.f32(rng.uniform(0, 1e-3, n))
    lr, b1, b2, eps, step = 2e-4, 0.9, 0.999, 1e-8, 7
    bufs = [G.dev(a) for a in (p0, g, m0, v0)]
    L.check(lib.bp_adam_step(*[L.ptr(b) for b in bufs], n, lr, b1, b2, eps, step, st), "adam_step")
    f = lambda x: float(np.float32(x))
    p_ref, m_ref, v_ref = R.adam(p0, g, m0, v0, f(lr), f(b1), f(b2), f(eps), step)
    within(host(bufs[2]), m_ref, 4 * U32 * (np.abs(m0) + 0.1 * np.abs(g)), "exp_avg")
    within(host(bufs[3]), v_ref, 4 * U32 * (v0 + g * g), "exp_avg_sq")
    within(host(bufs[0]), p_ref, 2 * ulp32(p_ref) + 8 * U32 * np.abs(p_ref - p0), "param")
    # the device-scalar form with the hyper-parameters laid out as optim.upload_hyper does: the same bits
    hyper = torch.tensor([lr, f(b1), f(b2), eps, 1.0 - math.pow(f(b1), step), math.sqrt(1.0 - math.pow(f(b2), step))],
                         dtype=torch.float32, device="cuda")
    bufs2 = [G.dev(a) for a in (p0, g, m0, v0)]
    L.check(lib.bp_adam_step_dev(*[L.ptr(b) for b in bufs2], n, L.ptr(hyper), st), "adam_step_dev")
    for a, b, what in zip(bufs, bufs2, ("param", "grad", "exp_avg", "exp_avg_sq")):
        same_bits(b, a, "adam_step_dev != adam_step: " + what)


def test_fill_and_sums_to_float():
    lib = L.load()
    st = G.stream()
    buf = torch.full((1000 + 7,), NAN, device="cuda")
    L.check(lib.bp_fill(L.ptr(buf), 1000, -2.5, st), "fill")
    b = host(buf)
    assert (b[:1000] == -2.5).all() and np.isnan(b[1000:]).all()
    sums = np.array([1.0 + 2 ** -30, -3.75, 1e-30, 3.4e38, 123456789.123], np.float64)
    sd = G.dev(sums, torch.float64)
    out = torch.full((6,), NAN, device="cuda")
    L.check(lib.bp_sums_to_float(L.ptr(sd), 5, L.ptr(out), st), "sums_to_float")
    o = out.cpu().numpy()
    assert np.array_equal(o[:5], sums.astype(np.float32)) and np.isnan(o[5])


def test_reductions_refuse_a_workspace_one_element_short():
    lib = L.load()
    st = G.stream()
    s = torch.zeros(3 * 1024, dtype=torch.float64, device="cuda")
    ws = workspace(1 << 24)
    for c, bf16, vargs in ((8, False, {}), (5, False, dict(cstride=8, coff=1)), (16, True, {})):
        xb, xv = upload(np.ones((2, 40, 40, c)), bf16, **vargs)
        nb = lib.bp_channel_sums_workspace(C.byref(xv))
        assert nb > 8
        assert lib.bp_channel_sums(C.byref(xv), L.ptr(s), L.ptr(ws), nb - 8, st) == L.BP_EWORKSPACE
        nb = lib.bp_act_backward_workspace(C.byref(xv))
        args = (C.byref(xv), None, C.byref(xv), None, None, None, L.ptr(s))
        assert lib.bp_act_backward(*args, L.ptr(ws), nb - 8, st) == L.BP_EWORKSPACE
        bf = L.BnBackwardFin(1.0, None, s.data_ptr(), s.data_ptr(), 1.0, None, None, s.data_ptr())
        assert lib.bp_act_backward_bn(*args, C.byref(bf), L.ptr(ws), nb - 8, st) == L.BP_EWORKSPACE
    ll = L.Loglik(2, 1, 1, 9, 13, 1, 0, 1.0, 1.0, 1.0)
    mb, mv = upload(np.ones((2, 9, 13, 1)))
    nb = lib.bp_loglik_workspace(C.byref(ll))
    out = torch.zeros(2 * 9 * 13 + 8, device="cuda")
    assert lib.bp_loglik_forward(C.byref(ll), L.ptr(out), C.byref(mv), None, None, L.ptr(out), None, L.ptr(out),
                                 L.ptr(ws), nb - 8, st) == L.BP_EWORKSPACE
    assert lib.bp_bce_logits(C.byref(mv), 0, 2, 1.0, L.ptr(s), L.ptr(ws), 256 * 8 - 8, st) == L.BP_EWORKSPACE
    assert lib.bp_l1_sum(C.byref(mv), L.ptr(out), L.ptr(s), L.ptr(ws), 256 * 8 - 8, st) == L.BP_EWORKSPACE
    lt = L.Latent(2, 1, 4, 96, 96, 0.0)                   # 73 728 elements: 256 blocks (the cap)
    qb, qv = upload(np.zeros((2, 96, 96, 8)))
    zb, zv = upload(np.zeros((2, 96, 96, 4)))
    st4 = torch.zeros(4 * 73728, device="cuda")
    assert lib.bp_latent_forward(C.byref(lt), C.byref(qv), None, None, None, L.ptr(zb), L.ptr(st4), C.byref(zv),
                                 L.ptr(s), L.ptr(ws), 256 * 8 - 8, st) == L.BP_EWORKSPACE
