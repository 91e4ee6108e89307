"""Device-side helpers shared by the GPU sweeps over tests/conv_sweep.py (plain module, no test in here): views that
are channel slices of wider buffers, the two criteria a stored tensor is judged by, and the per-case host operands.

test_gpu_conv_sweep.py runs every convolution implementation with them, test_gpu_stats_sweep.py the statistics
epilogues.  WORST collects the worst ratio to each limit over whatever ran in the process.
"""
import numpy as np
import torch

from baryon_painter_amd import _lib as L

import conv_sweep as S

TAGGED = S.tagged_cases()
U32 = 2.0 ** -24
TOL = {"y": 2e-5, "dx": 2e-5, "dw": 1e-4, "dbias": 1e-4}
TOL_BF16_STORED = 4e-3

WORST = {}                                                    # (criterion, impl, quantity) -> (ratio, case id)


def _layout(c, kind, bf16=False):
    """(cstride, coff) of a view of c channels: a 16-byte addressable slice, or one with odd stride and offset."""
    if kind == "aligned":
        q = 8 if bf16 else 4
        return (c + q - 1) // q * q + 8, q
    cs = c + 3
    return cs + (cs % 2 == 0), 1


def _in_view(a_nchw, kind, bf16=False):
    n, c, h, w = a_nchw.shape
    cs, co = _layout(c, kind, bf16)
    buf = torch.full((n, h, w, cs), 7.5, dtype=torch.float32, device="cuda")          # poison the unused channels
    buf[..., co:co + c] = torch.from_numpy(np.ascontiguousarray(a_nchw.transpose(0, 2, 3, 1))).cuda()
    if bf16:
        buf = buf.to(torch.bfloat16)
    return buf, L.View(buf.data_ptr(), n, h, w, c, cs, co, L.BF16 if bf16 else L.F32)


def _out_view(n, c, h, w, kind, bf16=False):
    cs, co = _layout(c, kind, bf16)
    buf = torch.full((n, h, w, cs), float("nan"), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    return buf, L.View(buf.data_ptr(), n, h, w, c, cs, co, L.BF16 if bf16 else L.F32)


def _read(buf, v):
    """(values of the view as float64 NCHW, True if every element outside the view is still NaN)."""
    f = buf.to(torch.float32)
    inside = f[..., v.coff:v.coff + v.c].permute(0, 3, 1, 2).contiguous().cpu().numpy().astype(np.float64)
    outside = torch.isnan(f[..., :v.coff]).all().item() and torch.isnan(f[..., v.coff + v.c:]).all().item()
    return inside, outside


def _half_ulp_bf16(a):
    _, ex = np.frexp(np.abs(a))
    return np.where(a == 0, 0.0, np.ldexp(1.0, ex - 9))


class Failures(list):
    def check(self, ok, msg):
        if not ok:
            self.append(msg)


def _judge(fails, cid, impl, q, got, ref, bnd, T, stored_bf16, where):
    """Both criteria for one result; records the worst ratio to each limit."""
    what = "%s %s [%s]" % (impl, q, where)
    if not np.isfinite(got).all():
        fails.append("%s: %d non-finite values inside the view" % (what, (~np.isfinite(got)).sum()))
        return
    err = np.abs(got - ref)
    tol = TOL_BF16_STORED if stored_bf16 else TOL[q]
    r1 = err.max() / max(np.abs(ref).max(), 1e-30) / tol
    lim = (np.broadcast_to(T, ref.shape) + 2.0) * U32 * bnd
    if stored_bf16:
        lim = lim + _half_ulp_bf16(np.abs(ref) + lim)
    # no product behind the element (a phase without a tap, an input row no output reads): the bias / zero, exactly --
    # selected by the count of products, so that a bias in the bound does not soften it
    exact = (lim == 0) | (np.broadcast_to(T, ref.shape) == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = np.where(exact, 0.0, err / np.where(exact, 1.0, lim)).max()
    for key, r in ((("max-relative", impl, q), r1), (("elementwise", impl, q), r2)):
        if r > WORST.get(key, (-1.0, ""))[0]:
            WORST[key] = (float(r), cid + " [" + where + "]")
    # (stored as bf16, "exactly the bias" is the bias rounded to bf16)
    want = S.bf16_round(ref.astype(np.float32)).astype(np.float64) if stored_bf16 else ref
    fails.check((got[exact] == want[exact]).all(), "%s: %d of %d elements without any product behind them are not exactly the bias / zero"
                % (what, (got[exact] != want[exact]).sum(), exact.sum()))
    fails.check(r2 <= 1.0, "%s: elementwise error %.3g of its derived limit (worst element %s)"
                % (what, r2, np.unravel_index(np.argmax(np.where(exact, 0.0, err / np.where(exact, 1.0, lim))), ref.shape)))
    fails.check(r1 <= 1.0, "%s: max error / max |ref| = %.3g, limit %.3g" % (what, r1 * tol, tol))


class Host:
    """Operands and float64 results of one case, computed once and shared by the impl x view loop."""

    def __init__(self, index):
        self.tag, self.case = TAGGED[index]
        self.biased = index % 3 == 0
        self.x, self.w, self.bias, self.dy, self.pw = S.make_inputs(self.case, index, self.biased)
        self.T = S.terms(self.case)
        self._f32, self._bf = None, {}

    def f32(self):
        if self._f32 is None:
            a = (self.case, self.x, self.w, self.bias, self.dy, self.pw)
            self._f32 = (S.reference(*a), S.bound(*a))
        return self._f32

    def bf16_operands(self, in_bf):
        """What the views hold: bf16 views hold rounded tensors, fp32 views the fp32 ones (the kernel rounds what it
        stages: act(x), dy)."""
        return (S.bf16_round(self.x), S.bf16_round(self.dy)) if in_bf else (self.x, self.dy)

    def bf16(self, in_bf):
        if in_bf not in self._bf:
            x, dy = self.bf16_operands(in_bf)
            a = (self.case, x, S.bf16_round(self.w), self.bias, S.bf16_round(dy), self.pw, S.bf16_round)
            self._bf[in_bf] = (S.reference(*a), S.bound(*a))
        return self._bf[in_bf]
