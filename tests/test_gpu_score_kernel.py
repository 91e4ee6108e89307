"""GPU: ``bp_loglik_samples`` and ``bp_posterior_score`` (csrc/score.hip) through the C ABI against the float64
restatements of tests/score_ref.py.

The limit of every comparison is 1e-12 of the sum of the magnitudes of the terms an entry adds up: the terms are float64
expressions of float32 inputs, a few ulp each from ``exp`` and from every addition of a tree that is a few thousand terms
deep, which comes to about 1e-14 of that sum; two orders of margin.  The effective sample size is an exponential of
differences of large numbers and is therefore checked against the device's OWN log-weights, within 1e-9 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as G
import score_ref as S
from baryon_painter_amd import _lib as L

pytestmark = pytest.mark.gpu
N = 3
SENT = -12345.0
PLANES = [(6, 10), (16, 16), (70, 36)]           # 60 pixels; one full wave's worth; two chunks with a ragged tail


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _heads(n, K, c, h, w, seed):
    rng = np.random.Generator(np.random.PCG64([seed, n, K, c, h, w]))
    x = (rng.random((n, c, h, w)) * 3.0).astype(np.float32)
    mu = (rng.standard_normal((K * n, c, h, w)) * 1.5 + 0.5).astype(np.float32)
    mu[0, 0, 0, :2] = (25.0, -30.0)                      # softplus: above its threshold, and where exp underflows to 1 + tiny
    lv = (rng.standard_normal((K * n, c, h, w)) - 1.5).astype(np.float32)
    return x, mu, lv


def _loglik(lib, x, mu, lv, K, softplus, cstride=None, coff=0, x_dev=None):
    """(out (K n, c), the float32 x_mu the kernel saw, return code) of one call; ``out`` is pre-filled with SENT."""
    n, c, h, w = x.shape
    ll = L.Loglik(n, K, c, h, w, softplus, 0 if lv is None else 1, 1.0, 1.0, 1.0)
    bm, vm = G.to_nhwc(mu, cstride, coff)
    bv, vv = G.to_nhwc(lv, cstride, coff) if lv is not None else (None, None)
    xd = G.dev(x) if x_dev is None else x_dev
    nbytes = lib.bp_loglik_samples_workspace(C.byref(ll))
    assert nbytes == K * n * c * ((h * w + 2047) // 2048) * 8
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    out = torch.full((K * n, c), SENT, dtype=torch.float64, device="cuda")
    rc = lib.bp_loglik_samples(C.byref(ll), L.ptr(xd), C.byref(vm), None if vv is None else C.byref(vv), L.ptr(out),
                               L.ptr(ws), nbytes, G.stream())
    x_mu = torch.empty((K * n, c, h, w), device="cuda")
    assert lib.bp_view_to_nchw(C.byref(vm), None, softplus, L.ptr(x_mu), G.stream()) == L.BP_OK
    torch.cuda.synchronize()
    for b in (bm, bv):                                   # the views were only read
        if b is not None and b.shape[-1] > c:
            assert bool((b[..., :coff] == 7.5).all()) and bool((b[..., coff + c:] == 7.5).all())
    return out.cpu().numpy(), x_mu.cpu().numpy(), rc


def _views(c):
    """(cstride, coff): a strided view, and the plain one (for one channel that is the 16-byte path)."""
    return [(4, 1), (None, 0)]


@pytest.mark.parametrize("h,w", PLANES + [(5, 7)])
@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_loglik_samples_equal_the_float64_restatement(K, c, h, w):
    """With and without a variance head, with and without softplus on the mean head, through a cstride = 4, coff = 1 view
    and a plain one -- for one channel and planes of a multiple of four pixels the 16-byte path; 5 x 7 is the one-channel
    plane that cannot take it.  For softplus the reference is fed x_mu as ``bp_view_to_nchw(softplus=1)`` returns it."""
    lib = L.load()
    x, mu, lv = _heads(N, K, c, h, w, seed=1)
    for with_var in (False, True):
        for softplus in (0, 1):
            outs = []
            for cstride, coff in _views(c):
                out, x_mu, rc = _loglik(lib, x, mu, lv if with_var else None, K, softplus, cstride, coff)
                assert rc == L.BP_OK
                if softplus:
                    assert x_mu[0, 0, 0, 0] == 25.0 and 0 < x_mu[0, 0, 0, 1] < 1e-12
                else:
                    assert np.array_equal(x_mu, mu)
                ref, mag = S.loglik_samples(x, x_mu, lv if with_var else None)
                err = np.abs(out - ref) / mag
                print(f"K={K} c={c} {h}x{w} var={with_var} softplus={softplus} cstride={cstride}: "
                      f"max |dev - ref| / sum|term| = {err.max():.3e}")
                assert (np.abs(out - ref) <= 1e-12 * mag).all(), (with_var, softplus, cstride, err.max())
                outs.append(out)
            # how a sample's pixels are split into partial sums depends on (h, w, c) alone: not on the view, not on the
            # path the loads take
            assert _same_bits(outs[0], outs[1]), (with_var, softplus)


@pytest.mark.parametrize("h,w", PLANES)
@pytest.mark.parametrize("c", [1, 2])
def test_loglik_samples_same_bits_again_alone_and_beside_a_nan(c, h, w):
    lib = L.load()
    K = 2
    x, mu, lv = _heads(N, K, c, h, w, seed=2)
    for cstride, coff in _views(c):
        a, _, rc = _loglik(lib, x, mu, lv, K, 1, cstride, coff)
        b, _, _ = _loglik(lib, x, mu, lv, K, 1, cstride, coff)
        assert rc == L.BP_OK and _same_bits(a, b)                           # two launches
        # sample l n + m launched alone (n = 1, K = 1) against x[m]
        for s in (0, 1 * N + 2):
            alone, _, rc = _loglik(lib, x[s % N:s % N + 1], mu[s:s + 1], lv[s:s + 1], 1, 1, cstride, coff)
            assert rc == L.BP_OK and _same_bits(alone[0], a[s]), (s, cstride)
        # a NaN planted in the last pixel of one sample's last channel, and one in another sample's variance head
        mu2, lv2 = mu.copy(), lv.copy()
        mu2[1 * N + 1, c - 1, h - 1, w - 1] = np.nan
        lv2[0 * N + 2, 0, 0, 0] = np.nan
        bad, _, rc = _loglik(lib, x, mu2, lv2, K, 1, cstride, coff)
        assert rc == L.BP_OK
        hit = np.zeros((K * N, c), bool)
        hit[1 * N + 1, c - 1] = hit[0 * N + 2, 0] = True
        assert np.isnan(bad[hit]).all() and _same_bits(bad[~hit], a[~hit])


def test_loglik_samples_from_a_pointer_off_the_16_byte_boundary():
    """x four bytes off: the scalar path, the same bits."""
    lib = L.load()
    h, w, K = 16, 16, 2
    x, mu, lv = _heads(N, K, 1, h, w, seed=3)
    a, _, _ = _loglik(lib, x, mu, lv, K, 0)
    flat = torch.zeros(N * h * w + 4, device="cuda")
    flat[1:1 + N * h * w] = G.dev(x).reshape(-1)
    b, _, rc = _loglik(lib, x, mu, lv, K, 0, x_dev=flat[1:])
    assert rc == L.BP_OK and _same_bits(a, b)


def test_loglik_samples_return_codes_leave_out_untouched():
    lib = L.load()
    n, K, c, h, w = N, 2, 2, 6, 10
    x, mu, lv = _heads(n, K, c, h, w, seed=4)
    xd = G.dev(x)
    bm, vm = G.to_nhwc(mu)
    bv, vv = G.to_nhwc(lv)
    ok = L.Loglik(n, K, c, h, w, 0, 1, 1.0, 1.0, 1.0)
    nbytes = lib.bp_loglik_samples_workspace(C.byref(ok))
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")
    out = torch.full((K * n, c), SENT, dtype=torch.float64, device="cuda")

    def call(ll=ok, x_=xd, m=vm, v=vv, o=out, w_=ws, nb=nbytes):
        return lib.bp_loglik_samples(None if ll is None else C.byref(ll), L.ptr(x_), None if m is None else C.byref(m),
                                     None if v is None else C.byref(v), L.ptr(o), L.ptr(w_), nb, G.stream())

    def desc(**kw):
        d = dict(n=n, L=K, c=c, h=h, w=w)
        d.update(kw)
        return L.Loglik(d["n"], d["L"], d["c"], d["h"], d["w"], 0, 1, 1.0, 1.0, 1.0)
    # BP_EINVAL: a null pointer other than var_raw
    assert call(ll=None) == call(x_=None) == call(m=None) == call(o=None) == call(w_=None) == L.BP_EINVAL
    # ... a malformed view (cstride < c; a null pointer inside; an unknown element type)
    assert call(m=L.View(bm.data_ptr(), K * n, h, w, c, c - 1, 0)) == L.BP_EINVAL
    assert call(v=L.View(None, K * n, h, w, c, c, 0)) == L.BP_EINVAL
    assert call(m=L.View(bm.data_ptr(), K * n, h, w, c, c, 0, 7)) == L.BP_EINVAL
    # ... n, L, c or an extent below 1
    for kw in ({"n": 0}, {"L": 0}, {"L": -1}, {"c": 0}, {"h": 0}, {"w": -3}):
        assert call(ll=desc(**kw)) == L.BP_EINVAL, kw
        assert lib.bp_loglik_samples_workspace(C.byref(desc(**kw))) == 0
    # ... mu_raw->n != n L, and view shapes that disagree with ll
    assert call(ll=desc(L=3)) == call(ll=desc(n=2)) == L.BP_EINVAL
    assert call(ll=desc(h=w, w=h)) == call(ll=desc(c=1)) == L.BP_EINVAL
    assert call(v=L.View(bv.data_ptr(), K * n, h, w, 1, c, 0)) == L.BP_EINVAL
    # BP_EUNSUPPORTED: a bf16 view
    half = torch.zeros((K * n, h, w, c), dtype=torch.bfloat16, device="cuda")
    assert call(m=L.View(half.data_ptr(), K * n, h, w, c, c, 0, L.BF16)) == L.BP_EUNSUPPORTED
    assert call(v=L.View(half.data_ptr(), K * n, h, w, c, c, 0, L.BF16)) == L.BP_EUNSUPPORTED
    # ... L > 64 (a view of 65 samples of one pixel), n L H W c = 2^31 (the geometry alone: nothing is launched)
    wide = torch.zeros((65, 1, 1, 1), device="cuda")
    assert call(ll=desc(n=1, L=65, c=1, h=1, w=1), m=L.View(wide.data_ptr(), 65, 1, 1, 1, 1, 0), v=None) \
        == L.BP_EUNSUPPORTED
    big = L.View(bm.data_ptr(), 1 << 14, 1 << 8, 1 << 8, 2, 2, 0)
    assert call(ll=desc(n=1 << 8, L=1 << 6, c=2, h=1 << 8, w=1 << 8), m=big, v=big) == L.BP_EUNSUPPORTED
    assert lib.bp_loglik_samples_workspace(C.byref(desc(n=1 << 8, L=1 << 6, c=2, h=1 << 8, w=1 << 8))) == 0
    # BP_EWORKSPACE
    assert call(nb=nbytes - 1) == call(nb=0) == L.BP_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ws == 0).all()) and bool((half == 0).all())
    # and the call itself is fine, with and without the variance head
    assert call() == L.BP_OK and call(v=None) == L.BP_OK
    torch.cuda.synchronize()
    assert not bool((out == SENT).any())


# ---------------------------------------------------------------------------------------------- bp_posterior_score
LATENTS = [(1, 2, 2), (1, 16, 16), (8, 1, 1)]
MZV = 1e-3


def _latent_case(K, dim_z, prior, dead, seed):
    """stats4 (4, N, *dim_z), eps (K, N, *dim_z), loglik (K N, 2).  Tile 1's log-likelihoods differ by 1e4 between
    draws (an unshifted logsumexp would overflow); with ``dead`` every draw of tile 2 is at -inf."""
    rng = np.random.Generator(np.random.PCG64([seed, K, *dim_z]))
    st = rng.standard_normal((4, N, *dim_z))
    st[1] -= 1.0
    if not prior:
        st[2:] = 0.0
    eps = rng.standard_normal((K, N, *dim_z))
    ll = rng.standard_normal((K, N, 2)) * 40.0 - 3000.0
    ll[:, 1, 0] += 1e4 * rng.permutation(K)
    if dead:
        ll[:, 2, 1] = -np.inf
    return st.astype(np.float32), eps.astype(np.float32), ll.reshape(K * N, 2)


def _score(lib, st, eps, ll, K, dim_z, want_log_w=True, c=2):
    lt = L.Latent(N, K, *dim_z, MZV)
    out = torch.full((N, 5), SENT, dtype=torch.float64, device="cuda")
    lw = torch.full((K, N), SENT, dtype=torch.float64, device="cuda") if want_log_w else None
    keep = (G.dev(st), G.dev(eps), G.dev(ll, torch.float64))
    rc = lib.bp_posterior_score(C.byref(lt), L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), c, L.ptr(out), L.ptr(lw),
                                G.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if lw is None else lw.cpu().numpy(), rc


def _close(dev, ref, limit):
    """Finite reference values within ``limit``; infinities and NaNs in the same places with the same sign."""
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        return bool((np.abs(dev - ref)[fin] <= np.broadcast_to(limit, ref.shape)[fin]).all()) and \
            np.array_equal(dev[~fin], ref[~fin], equal_nan=True)


@pytest.mark.parametrize("dim_z", LATENTS)
@pytest.mark.parametrize("K", [1, 2, 5, 17, 64])
def test_posterior_score_equals_the_float64_restatement(K, dim_z):
    lib = L.load()
    for prior in (True, False):
        for dead in (False, True):
            st, eps, ll = _latent_case(K, dim_z, prior, dead, seed=5)
            out, lw, rc = _score(lib, st, eps, ll, K, dim_z)
            assert rc == L.BP_OK
            r, r_mag = S.log_ratio(st[0], st[1], st[2], st[3], eps, np.float32(MZV))
            ll_sum = ll.sum(axis=1).reshape(K, N)
            lw_ref = ll_sum + r
            with np.errstate(invalid="ignore"):
                mag = np.maximum(1.0, np.where(np.isfinite(ll), np.abs(ll), 0.0).sum(axis=1).reshape(K, N) + r_mag)
            what = (K, dim_z, prior, dead)
            assert _close(lw, lw_ref, 1e-12 * mag), what
            ref = S.score(lw_ref, ll_sum, r)
            tile = 1e-12 * mag.max(axis=0)
            fin = np.isfinite(ref[:, :4])
            with np.errstate(invalid="ignore"):
                print(what, "max |dev - ref| / limit, columns 0-3:",
                      (np.abs(out[:, :4] - ref[:, :4])[fin] / np.broadcast_to(tile[:, None], (N, 4))[fin]).max())
            assert _close(out[:, :4], ref[:, :4], tile[:, None]), what
            # the effective sample size, from the device's own log-weights
            ess = S.ess_of(lw)
            live = np.isfinite(ess)
            assert (np.abs(out[live, 4] - ess[live]) <= 1e-9 * ess[live]).all(), what
            assert np.array_equal(np.isnan(out[:, 4]), np.isnan(ess))
            assert (out[live, 4] >= 1.0 - 1e-9).all() and (out[live, 4] <= K * (1.0 + 1e-9)).all()
            assert abs(out[1, 4] - 1.0) <= 1e-9            # tile 1: one draw carries all the weight
            if dead:
                assert np.isneginf(out[2, 0]) and np.isneginf(out[2, 1]) and np.isneginf(out[2, 2]) \
                    and np.isfinite(out[2, 3]) and np.isnan(out[2, 4])
            else:
                assert np.isfinite(out).all()
            assert (out[live, 0] >= out[live, 1] - 1e-12 * mag.max(axis=0)[live]).all()      # the bound tightens
            if K == 1:
                assert _same_bits(out[:, 0], out[:, 1]) and _same_bits(out[:, 0], lw[0])
                assert (out[live, 4] == 1.0).all()
            # without the log-weights: the same score
            out2, none, rc = _score(lib, st, eps, ll, K, dim_z, want_log_w=False)
            assert rc == L.BP_OK and none is None and _same_bits(out2, out)


def test_posterior_score_without_prior_planes_is_the_prior_sample_P_draws_from():
    """Zero prior planes: s_p = 1 + min_z_var, so r = sum[log s_q - log(1 + mzv) + eps^2/2 - (z / (1 + mzv))^2 / 2]."""
    lib = L.load()
    K, dim_z = 4, (1, 2, 2)
    st, eps, ll = _latent_case(K, dim_z, False, False, seed=6)
    out, lw, rc = _score(lib, st, eps, ll, K, dim_z)
    assert rc == L.BP_OK
    mzv = float(np.float32(MZV))
    sq = np.exp(st[1].astype(np.float64) / 2) + mzv
    z = st[0].astype(np.float64)[None] + eps.astype(np.float64) * sq[None]
    r = (np.log(sq)[None] - np.log1p(mzv) + 0.5 * eps.astype(np.float64) ** 2 - 0.5 * (z / (1 + mzv)) ** 2
         ).reshape(K, N, -1).sum(axis=2)
    assert np.allclose(lw, ll.sum(axis=1).reshape(K, N) + r, rtol=1e-13, atol=1e-10)
    assert np.allclose(out[:, 3], -r.mean(axis=0), rtol=1e-12, atol=1e-12)


def test_posterior_score_return_codes_leave_score_untouched():
    lib = L.load()
    K, dim_z = 4, (1, 2, 2)
    st, eps, ll = _latent_case(K, dim_z, True, False, seed=7)
    sd, ed, ld = G.dev(st), G.dev(eps), G.dev(ll, torch.float64)
    out = torch.full((N, 5), SENT, dtype=torch.float64, device="cuda")
    lw = torch.full((K, N), SENT, dtype=torch.float64, device="cuda")
    ok = L.Latent(N, K, *dim_z, MZV)

    def call(lt=ok, s=sd, e=ed, l_=ld, c=2, o=out, w_=lw):
        return lib.bp_posterior_score(None if lt is None else C.byref(lt), L.ptr(s), L.ptr(e), L.ptr(l_), c, L.ptr(o),
                                      L.ptr(w_), G.stream())
    assert call(lt=None) == call(s=None) == call(e=None) == call(l_=None) == call(o=None) == L.BP_EINVAL
    assert call(c=0) == call(c=-1) == L.BP_EINVAL
    for bad in ((0, K, 1, 2, 2), (N, 0, 1, 2, 2), (N, K, 0, 2, 2), (N, K, 1, 0, 2), (N, K, 1, 2, -1)):
        assert call(lt=L.Latent(*bad, MZV)) == L.BP_EINVAL, bad
    assert call(lt=L.Latent(N, 65, *dim_z, MZV)) == L.BP_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((lw == SENT).all())
    assert call() == L.BP_OK and call(w_=None) == L.BP_OK
    torch.cuda.synchronize()
    assert not bool((out == SENT).any()) and not bool((lw == SENT).any())
