"""GPU: the fully connected layer's entry points (bp_linear_forward / _backward_data / _backward_weight / _workspace,
csrc/linear.hip) through the C ABI against float64 NumPy.

Limits are those of tests/test_gpu_ops.py for the convolutions: forward and data gradient rel-L2 < 2e-5, weight gradient
< 1e-4, bias gradient < 1e-5 (a strictly sequential fp32 sum over K = 16 384 lies 2.6e-6 from float64: the forward limit
has seven-fold room over the worst summation order).  Shapes are the smallest that reach each code path: scalar and
16-byte weight loads, odd K, one and several slabs of the split over K, batches below / across / above one 32-row
matrix-core tile and more than two tiles, views inside wider buffers, (c, h, w) operands on either side."""
import ctypes as C

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import gpu_util as G

pytestmark = pytest.mark.gpu

SENT = -3.25


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-300)))


def chw(shape):
    return tuple(shape) if len(shape) == 3 else (shape[0], 1, 1)


def act64(x, pw):
    """float64 leaky(x * scale + shift, slope) per channel of an (n, c, h, w) array; ``pw`` None: identity."""
    x = np.asarray(x, np.float64)
    if pw is None:
        return x
    sc, sf, sl = (np.asarray(v, np.float64).reshape(1, -1, 1, 1) for v in pw)
    t = x * sc + sf
    return np.where(t > 0, t, t * sl)


class Case:
    """One layer on device buffers: x (n, c, h, w) in a (cs, co) buffer, W (O, K) [at a float offset], b, and y / dy
    (n, co, ho, wo) in a (cs, co) buffer."""

    def __init__(self, in_shape, in_cs, in_co, O, out_shape, out_cs, out_co, n, bias, pw, w_off=0, seed=3):
        rng = np.random.default_rng(seed)
        self.n, self.O = n, O
        self.ci, self.hi, self.wi = chw(in_shape)
        self.co, self.ho, self.wo = chw(out_shape)
        self.K = K = self.ci * self.hi * self.wi
        assert self.co * self.ho * self.wo == O
        self.x = rng.standard_normal((n, self.ci, self.hi, self.wi)).astype(np.float32)
        self.w = (rng.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32)
        self.b = rng.standard_normal(O).astype(np.float32) if bias else None
        self.dy = rng.standard_normal((n, self.co, self.ho, self.wo)).astype(np.float32)
        self.pw = None
        if pw:
            slopes = np.array([(0.0, 0.2, 1.0)[i % 3] for i in range(self.ci)], np.float32)
            self.pw = (rng.uniform(0.5, 1.5, self.ci).astype(np.float32),
                       (0.3 * rng.standard_normal(self.ci)).astype(np.float32), slopes)
        self.desc = L.Linear(K, O, self.ci, self.hi, self.wi, self.co, self.ho, self.wo, 1 if bias else 0)
        self.in_cs, self.in_co = in_cs or self.ci, in_co
        self.out_cs, self.out_co = out_cs or self.co, out_co
        self.xbuf, self.xv = G.to_nhwc(self.x, self.in_cs, self.in_co)
        self.dybuf, self.dyv = G.to_nhwc(self.dy, self.out_cs, self.out_co)
        self.wbuf = torch.zeros(O * K + w_off + 4, device="cuda")
        self.wd = self.wbuf[w_off:w_off + O * K]
        self.wd.copy_(torch.from_numpy(self.w.reshape(-1)))
        self.bd = None if self.b is None else G.dev(self.b)
        self.pwt, self.pws = (None, None) if self.pw is None else G.pointwise(*self.pw)
        self.lib = L.load()
        self.ws_bytes = int(self.lib.bp_linear_workspace(n, C.byref(self.desc)))
        self.ws = torch.zeros(self.ws_bytes // 4 + 4, device="cuda")
        # float64 references
        X = act64(self.x, self.pw).reshape(n, K)
        W = self.w.astype(np.float64)
        self.y_ref = (X @ W.T + (0 if self.b is None else self.b.astype(np.float64))).reshape(self.dy.shape)
        D = self.dy.astype(np.float64).reshape(n, O)
        self.dx_ref = (D @ W).reshape(self.x.shape)
        self.dw_ref = D.T @ X
        self.db_ref = D.sum(0)

    def pw_ref(self):
        return None if self.pws is None else C.byref(self.pws)

    def out_view(self, fill=SENT):
        buf = torch.full((self.n, self.ho, self.wo, self.out_cs), fill, dtype=torch.float32, device="cuda")
        return buf, L.View(buf.data_ptr(), self.n, self.ho, self.wo, self.co, self.out_cs, self.out_co)

    def in_view(self, fill=SENT):
        buf = torch.full((self.n, self.hi, self.wi, self.in_cs), fill, dtype=torch.float32, device="cuda")
        return buf, L.View(buf.data_ptr(), self.n, self.hi, self.wi, self.ci, self.in_cs, self.in_co)

    def forward(self):
        buf, v = self.out_view()
        rc = self.lib.bp_linear_forward(C.byref(self.desc), C.byref(self.xv), self.pw_ref(), L.ptr(self.wd),
                                        L.ptr(self.bd), C.byref(v), L.ptr(self.ws), self.ws_bytes, G.stream())
        return rc, buf

    def backward_data(self):
        buf, v = self.in_view()
        rc = self.lib.bp_linear_backward_data(C.byref(self.desc), C.byref(self.dyv), L.ptr(self.wd), C.byref(v),
                                              G.stream())
        return rc, buf

    def backward_weight(self):
        g = 8                                                       # guard floats on either side
        dw = torch.full((self.O * self.K + 2 * g,), SENT, device="cuda")
        db = torch.full((self.O + 2 * g,), SENT, device="cuda")
        rc = self.lib.bp_linear_backward_weight(C.byref(self.desc), C.byref(self.xv), self.pw_ref(), C.byref(self.dyv),
                                                L.ptr(dw[g:]), None if self.b is None else L.ptr(db[g:]), G.stream())
        return rc, dw, db, g


def untouched(buf, c, coff):
    other = np.ones(buf.shape[-1], bool)
    other[coff:coff + c] = False
    return bool((buf.cpu().numpy()[..., other] == SENT).all())


# (input (c,h,w) | (d,), its buffer's channel stride / offset, O, output shape, its stride / offset, n, bias, pending
#  pointwise on the input, float offset of W in its buffer)
CASES = {
    "odd-K-scalar-n3": ((3, 5, 5), 7, 1, 24, (6, 2, 2), 16, 4, 3, True, True, 0),           # unflatten (2,3,2,2)
    "odd-K-O1-n1": ((3, 5, 5), 7, 1, 1, (1,), None, 0, 1, False, False, 0),
    "odd-K-mfma-n70": ((3, 5, 5), 7, 1, 40, (40,), None, 0, 70, True, True, 0),
    "fixture-n3": ((64, 2, 2), None, 0, 8, (2, 2, 2), None, 0, 3, True, True, 0),
    "fixture-O40-n33": ((64, 2, 2), None, 0, 40, (40,), None, 0, 33, True, False, 0),
    "fixture-unaligned-W-n33": ((64, 2, 2), None, 0, 24, (6, 2, 2), 16, 4, 33, False, True, 1),
    "bottleneck-K16384-n3": ((64, 16, 16), None, 0, 8, (2, 2, 2), None, 0, 3, True, True, 0),
    "bottleneck-K16384-n70": ((64, 16, 16), None, 0, 8, (8,), None, 0, 70, True, False, 0),
    "flat12-n70": ((12,), None, 0, 24, (6, 2, 2), 16, 4, 70, False, True, 0),
    "flat12-O40-n1": ((12,), None, 0, 40, (40,), None, 0, 1, True, False, 0),
    "flat12-O4-n33": ((12,), None, 0, 4, (1, 2, 2), 4, 1, 33, True, False, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_linear_against_float64(name):
    cs = Case(*CASES[name])
    assert cs.ws_bytes > 0
    # forward
    rc, ybuf = cs.forward()
    assert rc == L.BP_OK
    y = G.from_nhwc(ybuf, cs.co, cs.out_co)
    e = rel_l2(y, cs.y_ref)
    print(name, "forward", e)
    assert e < 2e-5
    assert untouched(ybuf, cs.co, cs.out_co)
    rc, again = cs.forward()
    assert rc == L.BP_OK and torch.equal(again, ybuf)                          # the same bits
    # data gradient
    rc, dxbuf = cs.backward_data()
    assert rc == L.BP_OK
    e = rel_l2(G.from_nhwc(dxbuf, cs.ci, cs.in_co), cs.dx_ref)
    print(name, "backward_data", e)
    assert e < 2e-5
    assert untouched(dxbuf, cs.ci, cs.in_co)
    rc, again = cs.backward_data()
    assert rc == L.BP_OK and torch.equal(again, dxbuf)
    # weight and bias gradient, torch layout
    rc, dw, db, g = cs.backward_weight()
    assert rc == L.BP_OK
    dwh, dbh = dw.cpu().numpy(), db.cpu().numpy()
    e = rel_l2(dwh[g:-g].reshape(cs.O, cs.K), cs.dw_ref)
    print(name, "backward_weight", e)
    assert e < 1e-4
    assert (dwh[:g] == SENT).all() and (dwh[-g:] == SENT).all()
    if cs.b is not None:
        e = rel_l2(dbh[g:-g], cs.db_ref)
        print(name, "bias gradient", e)
        assert e < 1e-5
        assert (dbh[:g] == SENT).all() and (dbh[-g:] == SENT).all()
    else:
        assert (dbh == SENT).all()
    rc, dw2, db2, _ = cs.backward_weight()
    assert rc == L.BP_OK and torch.equal(dw2, dw) and torch.equal(db2, db)


def test_bad_arguments_are_refused_before_anything_is_written():
    cs = Case(*CASES["bottleneck-K16384-n3"])
    lib = cs.lib
    assert cs.ws_bytes == 64 * 3 * 8 * 4                  # 64 slabs of 256 features: the split over K
    ybuf, yv = cs.out_view()

    def fwd(desc, xv, yv, nbytes, w=cs.wd, b=cs.bd):
        return lib.bp_linear_forward(C.byref(desc), C.byref(xv), cs.pw_ref(), L.ptr(w), L.ptr(b), C.byref(yv),
                                     L.ptr(cs.ws), nbytes, G.stream())
    assert fwd(cs.desc, cs.xv, yv, cs.ws_bytes - 1) == L.BP_EWORKSPACE
    wrong = L.Linear(cs.K - 1, cs.O, cs.ci, cs.hi, cs.wi, cs.co, cs.ho, cs.wo, 1)
    assert fwd(wrong, cs.xv, yv, cs.ws_bytes) == L.BP_EINVAL
    other = L.Linear(cs.K, cs.O, cs.ci, cs.hi, cs.wi, cs.O, 1, 1, 1)               # the view is (2, 2, 2)
    assert fwd(other, cs.xv, yv, cs.ws_bytes) == L.BP_EINVAL
    x0 = L.View(cs.xbuf.data_ptr(), 0, cs.hi, cs.wi, cs.ci, cs.in_cs, cs.in_co)
    y0 = L.View(ybuf.data_ptr(), 0, cs.ho, cs.wo, cs.co, cs.out_cs, cs.out_co)
    assert fwd(cs.desc, x0, y0, cs.ws_bytes) == L.BP_EINVAL
    y2 = L.View(ybuf.data_ptr(), 2, cs.ho, cs.wo, cs.co, cs.out_cs, cs.out_co)      # batch sizes differ
    assert fwd(cs.desc, cs.xv, y2, cs.ws_bytes) == L.BP_EINVAL
    assert fwd(cs.desc, cs.xv, yv, cs.ws_bytes, b=None) == L.BP_EINVAL              # has_bias without a bias
    assert lib.bp_linear_forward(C.byref(cs.desc), C.byref(cs.xv), None, None, L.ptr(cs.bd), C.byref(yv), L.ptr(cs.ws),
                                 cs.ws_bytes, G.stream()) == L.BP_EINVAL
    assert lib.bp_linear_workspace(0, C.byref(cs.desc)) == 0 and lib.bp_linear_workspace(3, C.byref(wrong)) == 0
    torch.cuda.synchronize()
    assert (ybuf == SENT).all()
    # the gradients
    dxbuf, dxv = cs.in_view()
    assert lib.bp_linear_backward_data(C.byref(wrong), C.byref(cs.dyv), L.ptr(cs.wd), C.byref(dxv), G.stream()) == L.BP_EINVAL
    dx0 = L.View(dxbuf.data_ptr(), 0, cs.hi, cs.wi, cs.ci, cs.in_cs, cs.in_co)
    assert lib.bp_linear_backward_data(C.byref(cs.desc), C.byref(cs.dyv), L.ptr(cs.wd), C.byref(dx0), G.stream()) == L.BP_EINVAL
    assert lib.bp_linear_backward_data(C.byref(cs.desc), C.byref(cs.dyv), None, C.byref(dxv), G.stream()) == L.BP_EINVAL
    dw = torch.full((cs.O * cs.K,), SENT, device="cuda")
    db = torch.full((cs.O,), SENT, device="cuda")
    assert lib.bp_linear_backward_weight(C.byref(wrong), C.byref(cs.xv), None, C.byref(cs.dyv), L.ptr(dw), L.ptr(db),
                                         G.stream()) == L.BP_EINVAL
    assert lib.bp_linear_backward_weight(C.byref(cs.desc), C.byref(x0), None, C.byref(cs.dyv), L.ptr(dw), L.ptr(db),
                                         G.stream()) == L.BP_EINVAL
    assert lib.bp_linear_backward_weight(C.byref(cs.desc), C.byref(cs.xv), None, C.byref(cs.dyv), None, L.ptr(db),
                                         G.stream()) == L.BP_EINVAL
    torch.cuda.synchronize()
    assert (dxbuf == SENT).all() and (dw == SENT).all() and (db == SENT).all()


@pytest.mark.parametrize("n", [3, 33])
def test_prelu_behind_a_linear_layer(n):
    """The slope gradient of a PReLU on the flat (n, 1, 1, O) output: bp_act_backward's third sum through
    bp_prelu_slope_grad, and g = dout * act'(raw) in place, against float64."""
    cs = Case((64, 2, 2), None, 0, 40, (40,), None, 0, n, True, False, 0, seed=11)
    lib, O, a = cs.lib, cs.O, 0.25
    rc, ybuf = cs.forward()
    assert rc == L.BP_OK
    yv = L.View(ybuf.data_ptr(), n, 1, 1, O, O, 0)
    raw = ybuf.cpu().numpy().astype(np.float64).reshape(n, O)
    assert rel_l2(raw, cs.y_ref.reshape(n, O)) < 2e-5
    _, pws = pw = G.pointwise(np.ones(O), np.zeros(O), np.full(O, a))
    dout = np.random.default_rng(5).standard_normal((n, O)).astype(np.float32)
    dbuf = G.dev(dout.reshape(n, 1, 1, O))
    dv = L.View(dbuf.data_ptr(), n, 1, 1, O, O, 0)
    sums = torch.zeros(3 * O, dtype=torch.float64, device="cuda")
    nb = int(lib.bp_act_backward_workspace(C.byref(yv)))
    ws = torch.zeros(nb // 8 + 32, dtype=torch.float64, device="cuda")
    L.check(lib.bp_act_backward(C.byref(dv), None, C.byref(yv), C.byref(pws), None, C.byref(dv), L.ptr(sums), L.ptr(ws),
                                ws.numel() * 8, G.stream()), "act backward")
    dslope = torch.zeros(1, device="cuda")
    L.check(lib.bp_prelu_slope_grad(L.ptr(sums), O, L.ptr(dslope), G.stream()), "prelu slope grad")
    d64 = dout.astype(np.float64)
    ref = (d64 * raw * (raw <= 0)).sum()
    assert abs(float(dslope) - ref) <= 1e-5 * abs(ref), (float(dslope), ref)
    g_ref = d64 * np.where(raw > 0, 1.0, a)
    assert rel_l2(dbuf.cpu().numpy().reshape(n, O), g_ref) < 1e-6
    del pw
