"""GPU: ``bp_likelihood_draw`` through the C ABI against the oracle's Philox lattice and the float32 restatement of the
draw (tests/pixel_noise_ref.py): strided views, workgroups that straddle tiles (hw = 96), a channel count that crosses a
group of four, 64-bit seeds and ids, the shared lattice, untouched bytes and every return code."""
import ctypes as C

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import gpu_util as G
import pixel_noise_ref as R

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 17
IDS = np.array([0, 2 ** 33 + 5, 123456789012], dtype=np.int64)
ORIGINS = np.array([(3, 7), (0, 1000), (2 ** 20 + 1, 2 ** 23 + 5)], dtype=np.int32)
SHAPES = [(h, w, c) for (h, w) in ((8, 12), (16, 16)) for c in (1, 3, 5, 8)]
N = 3


def draw(mu, lv, softplus, ids=IDS, origins=ORIGINS, seed=SEED):
    """``bp_likelihood_draw`` on NCHW arrays laid out as strided NHWC views (sources: cstride c + 3, coff 2; destination:
    cstride c + 1, coff 1).  Returns (out NCHW, the three buffers, copies of the source buffers as they were)."""
    lib = L.load()
    n, c, h, w = mu.shape
    bm, vm = G.to_nhwc(mu, c + 3, 2)
    bl, vl = G.to_nhwc(lv, c + 3, 2)
    bo, vo = G.to_nhwc(np.zeros_like(mu), c + 1, 1)
    before = (bm.clone(), bl.clone())
    seed_d = torch.from_numpy(np.array([seed], dtype=np.uint64).view(np.int64)).cuda()
    ids_d = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    org_d = None if origins is None else torch.from_numpy(np.ascontiguousarray(origins)).cuda()
    L.check(lib.bp_likelihood_draw(C.byref(vm), softplus, C.byref(vl), L.ptr(seed_d), L.ptr(ids_d), L.ptr(org_d),
                                   C.byref(vo), G.stream()), "likelihood draw")
    torch.cuda.synchronize()
    return G.from_nhwc(bo, c, 1), (bm, bl, bo), before


def nchw(e):
    return np.ascontiguousarray(e.transpose(0, 3, 1, 2))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_unit_draws_are_the_oracles_lattice_normals():
    """mu = 0, log_var = 0: out is e.  The project's condition for bp_philox_normal, pooled over all shapes: libm may
    differ in a last bit."""
    worst, equal, total = 0.0, 0, 0
    for h, w, c in SHAPES:
        z = np.zeros((N, c, h, w), np.float32)
        got, _, _ = draw(z, z, 0)
        ref = nchw(R.lattice_normals(SEED, IDS, ORIGINS, h, w, c))
        worst = max(worst, float(np.abs(got - ref).max()))
        equal += int((got == ref).sum())
        total += ref.size
    print("max difference", worst, "equal fraction", equal / total)
    assert worst <= 2.0 ** -22 and equal / total > 0.999


def test_zero_variance_returns_the_mean_bit_for_bit():
    """log_var = -inf: out equals bp_view_to_nchw(mu, softplus), NaN, values above the softplus threshold and -0.0
    included."""
    lib = L.load()
    rng = np.random.Generator(np.random.PCG64(41))
    for h, w, c in SHAPES:
        mu = (rng.standard_normal((N, c, h, w)) * 8).astype(np.float32)
        flat = mu.reshape(-1)
        flat[::7] = -0.0
        flat[3::11] = np.nan
        flat[5::13] = 25.0
        flat[6::17] = 100.0
        flat[2::19] = 20.0
        lv = np.full_like(mu, -np.inf)
        for softplus in (0, 1):
            got, (bm, _, _), _ = draw(mu, lv, softplus)
            ref = torch.zeros((N, c, h, w), device="cuda")
            vm = L.View(bm.data_ptr(), N, h, w, c, c + 3, 2)
            L.check(lib.bp_view_to_nchw(C.byref(vm), None, softplus, L.ptr(ref), G.stream()))
            assert np.array_equal(bits(got), bits(ref.cpu().numpy())), (h, w, c, softplus)


def test_draws_equal_the_float32_restatement():
    """log_var uniform in [-12, 4]: |got - ref| <= 2^-21 |p| + 2^-23 |ref| per element (pixel_noise_ref.draw_bound).
    t is the device's own bp_view_to_nchw(mu, softplus), which the zero-variance test pins bit for bit: the bound
    speaks of expf, the product and the sum, not of libm's log1p."""
    lib = L.load()
    rng = np.random.Generator(np.random.PCG64(42))
    worst = 0.0
    for h, w, c in SHAPES:
        mu = (rng.standard_normal((N, c, h, w)) * 3).astype(np.float32)
        lv = rng.uniform(-12, 4, (N, c, h, w)).astype(np.float32)
        e = nchw(R.lattice_normals(SEED, IDS, ORIGINS, h, w, c))
        for softplus in (0, 1):
            got, (bm, _, _), _ = draw(mu, lv, softplus)
            t = torch.zeros((N, c, h, w), device="cuda")
            vm = L.View(bm.data_ptr(), N, h, w, c, c + 3, 2)
            L.check(lib.bp_view_to_nchw(C.byref(vm), None, softplus, L.ptr(t), G.stream()))
            ref, p = R.draw_ref(t.cpu().numpy(), lv, e)
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            bound = R.draw_bound(ref, p)
            # the figure to report: the error in units of the one-ulp-of-expf bound 2^-22 |p| + 2^-23 |ref|
            worst = max(worst, float((err / (2.0 ** -22 * np.abs(p.astype(np.float64))
                                             + 2.0 ** -23 * np.abs(ref.astype(np.float64)) + 1e-300)).max()))
            assert (err <= bound).all(), (h, w, c, softplus, float((err / np.maximum(bound, 1e-300)).max()))
    print("worst error / (2^-22 |p| + 2^-23 |ref|):", worst)


def test_tiles_of_one_id_share_the_lattice():
    h, w, c = 16, 16, 5
    z = np.zeros((N, c, h, w), np.float32)
    ids = np.array([2 ** 33 + 5, 2 ** 33 + 5, 9], dtype=np.int64)
    org = np.array([(0, 0), (5, 6), (0, 0)], dtype=np.int32)
    got, _, _ = draw(z, z, 0, ids=ids, origins=org)
    assert np.array_equal(bits(got[0, :, 5:, 6:]), bits(got[1, :, :11, :10]))
    assert not np.array_equal(got[0], got[1]) and (got[2] == got[0]).mean() < 0.01
    # null origins are zero origins
    zero, _, _ = draw(z, z, 0, ids=ids, origins=None)
    assert np.array_equal(bits(zero[0]), bits(got[0])) and np.array_equal(bits(zero[2]), bits(got[2]))
    assert np.array_equal(bits(zero[1]), bits(zero[0]))
    # another key: another lattice
    other, _, _ = draw(z, z, 0, ids=ids, origins=org, seed=SEED + 1)
    assert (other == got).mean() < 0.01


def test_bytes_outside_the_views_are_untouched():
    rng = np.random.Generator(np.random.PCG64(43))
    for h, w, c in SHAPES:
        mu = rng.standard_normal((N, c, h, w)).astype(np.float32)
        lv = rng.uniform(-3, 1, (N, c, h, w)).astype(np.float32)
        got, (bm, bl, bo), (bm0, bl0) = draw(mu, lv, 1)
        assert torch.equal(bm, bm0) and torch.equal(bl, bl0)
        outside = torch.ones(c + 1, dtype=torch.bool, device="cuda")
        outside[1:1 + c] = False
        assert (bo[..., outside] == 7.5).all() and np.isfinite(got).all() and (got != 0).all()


def test_return_codes_come_before_any_launch():
    lib = L.load()
    n, h, w, c = 2, 4, 4, 3
    x = np.zeros((n, c, h, w), np.float32)
    bm, vm = G.to_nhwc(x, c + 3, 2)
    bl, vl = G.to_nhwc(x, c + 3, 2)
    bo, vo = G.to_nhwc(x, c + 1, 1)
    bo.fill_(7.5)
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    ids = torch.zeros(n, dtype=torch.int64, device="cuda")
    org = torch.zeros((n, 2), dtype=torch.int32, device="cuda")

    def call(mu=vm, lv=vl, out=vo, s=seed, i=ids, o=org):
        rc = lib.bp_likelihood_draw(None if mu is None else C.byref(mu), 0, None if lv is None else C.byref(lv),
                                    L.ptr(s), L.ptr(i), L.ptr(o), None if out is None else C.byref(out), G.stream())
        torch.cuda.synchronize()
        assert (bo == 7.5).all()
        return rc

    def view(buf, **kw):
        d = dict(n=n, h=h, w=w, c=c, cstride=buf.shape[-1], coff=1, dtype=L.F32)
        d.update(kw)
        return L.View(buf.data_ptr(), d["n"], d["h"], d["w"], d["c"], d["cstride"], d["coff"], d["dtype"])

    # BP_EINVAL: a null pointer other than origins, a malformed view, views that differ in n, h, w or c
    for kw in (dict(mu=None), dict(lv=None), dict(out=None), dict(s=None), dict(i=None)):
        assert call(**kw) == L.BP_EINVAL, kw
    assert call(out=view(bo, coff=2)) == L.BP_EINVAL                         # coff + c > cstride
    assert call(mu=view(bm, c=0)) == L.BP_EINVAL
    assert call(lv=L.View(0, n, h, w, c, c + 3, 2)) == L.BP_EINVAL           # a null data pointer
    for kw in (dict(n=1), dict(h=2), dict(w=2), dict(c=2)):
        assert call(out=view(bo, **kw)) == L.BP_EINVAL, kw
        assert call(lv=view(bl, **kw)) == L.BP_EINVAL, kw
    # BP_EUNSUPPORTED: a bf16 view; n h w c >= 2^31 (never launched: the views only claim the size)
    for name in ("mu", "lv", "out"):
        buf = {"mu": bm, "lv": bl, "out": bo}[name]
        assert call(**{name: view(buf, dtype=L.BF16)}) == L.BP_EUNSUPPORTED, name
    big = dict(n=2 ** 11, h=2 ** 10, w=2 ** 10, c=1, cstride=1, coff=0)
    assert call(mu=view(bm, **big), lv=view(bl, **big), out=view(bo, **big)) == L.BP_EUNSUPPORTED
    # ... and the call that is in order, with null origins
    assert lib.bp_likelihood_draw(C.byref(vm), 0, C.byref(vl), L.ptr(seed), L.ptr(ids), None, C.byref(vo),
                                  G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    assert (bo[..., 1:1 + c] != 7.5).all() and (bo[..., 0] == 7.5).all()
