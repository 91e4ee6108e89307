"""GPU: the statistics epilogues of every convolution kernel family, swept over the geometries of tests/conv_sweep.py.

Training takes every batch-norm statistic and every activation-backward reduction from a sum fused into a convolution
kernel's epilogue (bp_conv_forward_stats, bp_conv_forward_bn, bp_conv_backward_data_stats, bp_conv_backward_data_act),
and each kernel family has its own copy of that epilogue.  test_gpu_epilogue_stats.py and test_gpu_bf16_ops.py run them
at 29 hand-picked layers against a limit of 2e-5 (or 1e-6) of the sum of magnitudes, which cannot see one dropped or
doubled pixel among 10^6.  Here the 753 pinned cases of the convolution sweep and conv_sweep.STATS_EXTRA (row-count
regimes of the first fold, 256 / 512 produced channels, every register-resident family past its grid-stride or fold
threshold) run through all four entry points and are judged by exactness.

Configurations per case: 16-byte addressable ("aligned") and odd-stride ("odd") channel slices of wider buffers;
BP_IMPL_MFMA forward and data gradient; BP_IMPL_BF16 forward with bf16 and with fp32 views; the bf16 data gradient;
bp_conv_backward_data_act in fp32 and bf16; the `raw` view of the data gradient in the views' layout and, on the aligned
runs, once more in the odd one (both branches of raw_vec); the ws:* cases with bp_set_option on and off.  Destinations,
sums and the workspace with 8 guard doubles behind it are pre-filled with NaN.

Return codes, ws = bp_conv_stats_workspace / bp_conv_backward_data_act_workspace for the very views of the call:
ws = 0: BP_EUNSUPPORTED, destination and sums still all NaN.  ws > 0: BP_OK -- and with workspace_bytes = ws - 8
BP_EWORKSPACE, nothing written.  After BP_OK every channel outside the view and the guard doubles are still NaN and no
element of sums is (an idle workgroup that skipped its zero row would leave one).

Judgement, two operand sets:
 (a) conv_sweep.counting_inputs: every value a small integer or half-integer.  With Q, the per-channel sum of |term| in
     units of the terms' grid (sum y^2; 4 sum |g raw| and 4 sum |dx t|), below 2^24 every possible accumulation -- fp32 or
     double, any order -- is exact: the stored tensor equals the reference bit for bit and every sum equals the
     reference sum exactly.  No tolerance.  Q >= 2^24 skips this check only; at most 5 % of the BP_OK calls may.
 (b) the sweep's own operands (make_inputs, no bias; raw redrawn where |t| < 1e-3): the stored tensor through the
     convolution sweep's two criteria, unchanged; the sums against the float64 sums OF THE TENSOR THE CALL STORED, which
     takes the convolution's own rounding out of the comparison, within the limits of test_gpu_pointwise.py:
       1e-12 sum|term|            kernels that accumulate exact terms in double (every fp32 family but those of fp32_run below)
       2e-6 sum|term|             the bf16 kernels, which add short groups in fp32 first
       F 2^-24 sum|term|          fp32 families with an fp32 run of F terms before the double accumulators (fp32_run).
     The bf16 head kernel of bp_conv_backward_data_act sums the unrounded gradient while the reference has the stored,
     bf16-rounded one: its limit carries the half bf16 ulp of every term the reference rounds.
bp_conv_forward_bn equals bp_conv_forward_stats + bp_bn_finalize bit for bit (the nine outputs) on every forward case
with a workspace on aligned fp32 views.

Recorded on one MI355X, the whole file (778 cases + the report, 45 s against 65 s of test_gpu_conv_sweep.py in the same
visit; nothing thinned).  Calls, BP_OK / BP_EUNSUPPORTED: forward_stats 1430 / 1706, forward_stats bf16 1100 / 2404,
backward_data_stats 2064 / 2640, bf16 32 / 2116, backward_data_act 28 / 3108, bf16 6 / 1426, forward_bn 365 / 0; no other
code.  Exact checks: 2328 made, 2 skipped of 2330.  Worst ratio to each limit for the sums: 1e-12: 2e-4 (grid:410);
2e-6 (bf16): 0.16 (gate:small_8_1_k5, the head kernel); F 2^-24: 0.69 (gate:enc_8_16, F = 1), 0.14 (gate:enc0_1_8, F = 4),
0.09 (ext:in1x1_k7, F = 8), 0.002 (gate:small_8_1_k5, F = 256).  Stored tensors: fp32 0.58 elementwise / 0.19 max-relative,
bf16 1.00 / 0.94 of their limits.  Found and fixed (conv_sweep.STATS_REGRESSIONS): the workspace queries of conv_flat.hip's
three forward kernels answered for views the kernels refuse; its k7 data gradient refused a raw view that is not 16-byte
addressable after a non-zero query; the bf16 weights-stationary forward ran with a workspace 8 bytes short of the query.
No sum of any family was wrong.
"""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L
from oracle import ops

import conv_sweep as S
import gpu_util as G
from conv_sweep_gpu import WORST as CONV_WORST, Failures, _in_view, _judge, _out_view, _read

pytestmark = pytest.mark.gpu

# seconds of `pytest -m gpu` for this file / for tests/test_gpu_conv_sweep.py, measured in the same visit on one MI355X
WALL_TIME = {"test_gpu_stats_sweep.py": 45, "test_gpu_conv_sweep.py": 65}

TAGGED = S.stats_cases()
NAN = float("nan")
TWO24 = 2.0 ** 24
U32 = 2.0 ** -24

# bp_set_option switches between a special kernel and the tiled one: layers they apply to (both settings are run), as in
# test_gpu_conv_sweep.py -- the ws:* cases and whatever else sits on these layers
SWITCHES = {
    (0, 128, 128, 3, 1, 1, 0): (b"f32_ws", b"bf16_ws"),
    (0, 64, 128, 4, 2, 1, 0): (b"bf16_ws",),
    (1, 128, 64, 4, 2, 1, 0): (b"bf16_ws",),
}

# fp32 families that add in fp32 before their double accumulators: the longest fp32 run F of one call, read from the kernel
#   760000          conv_enc.hip:114-173 enc_fwd_kernel: a thread adds its one pixel of every tile its workgroup walks
#                   (ssum / ssq), grid of min(tiles, 512) workgroups (conv_enc.hip:638-644): F = ceil(tiles / grid)
#   780001, 780002  conv_enc.hip:415-455 enc0_fwd_kernel: a thread's 2 x 2 pixels of every tile, grid of min(tiles, 2048)
#                   (conv_enc.hip:647-654): F = 4 ceil(tiles / grid)
#   710000          conv_flat.hip:120-160 flat_k7_kernel (data gradient): a wave's 8 pixel groups of one tile in fp32 (ps),
#                   added to the lane's double after every tile: F = 8
#   small           conv_small.hip:243-259 small_conv_kernel<ACT>: a thread's 4 pixels and a wave's 64 columns: F = 256
# Every other fp32 family keeps its sums in double from the accumulators on (conv_igemm.hip:114-118, conv_stem.hip,
# conv_flat.hip, conv_ws_f32.hip:158-175, conv_small.hip:386-398 for the one-channel kernels).
def fp32_run(family, case):
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    if family == "760000":
        tiles = n * -(-wo // 16) * -(-ho // 4)
        return -(-tiles // min(tiles, 512))
    if family in ("780001", "780002"):
        tiles = n * -(-wo // 32) * -(-ho // 8)
        return 4 * -(-tiles // min(tiles, 2048))
    if family == "710000":
        return 8
    if family == "small":
        return 256
    return 0


LIMIT_DOUBLE, LIMIT_BF16 = 1e-12, 2e-6

FWD_FAMILIES = ("plain-mt1", "plain-mt4", "dma4", "dma8", "dmaf", "wres", "700000", "720000", "730000", "740000", "760000",
                "780001", "780002", "tiny")
BWD_FAMILIES = ("plain-mt1", "plain-mt4", "dma4", "dma8", "dmaf", "710000")
TILED = ("plain-mt1", "plain-mt4", "dma4", "dma8", "dmaf", "wres")

OUTCOMES = collections.defaultdict(collections.Counter)       # entry point -> {return code: calls}
SERVED = collections.Counter()                                # (direction, family) -> BP_OK calls, BP_IMPL_MFMA aligned
REGIMES = collections.Counter()                               # (direction, fold regime) -> BP_OK calls of the tiled kernels
EXACT = collections.Counter()                                 # "made" / "skipped" exact checks, "ok" counting calls
WORST = {}                                                    # (entry, limit) -> (ratio, case id)
BN_COMPARED = [0]
RAN = set()


# ---------------------------------------------------------------------------------------------------------- host side
def _conv_fwd(case, xa, w):
    tr, ci, co, k, s, p, op = case[:7]
    return ops.convT2d_fwd(xa, w, s, p, op) if tr else ops.conv2d_fwd(xa, w, s, p)


def _conv_dgrad(case, dy, w):
    tr, ci, co, k, s, p, op, n, h, wd = case
    return ops.convT2d_bwd_data(dy, w, s, p)[:, :, :h, :wd] if tr else ops.conv2d_bwd_data(dy, w, s, p, h, wd)


def _draw_raw(rng, shape, scale, shift, bf16):
    """raw with |fma(raw, scale, shift)| >= 1e-3, so that the fp32 mask is unambiguous (as tests/test_gpu_pointwise.py)."""
    rnd = S.bf16_round if bf16 else (lambda a: np.asarray(a, np.float32))
    raw = rnd((rng.standard_normal(shape) * 1.3).astype(np.float32)).copy()
    sc, sf = scale[None, :, None, None].astype(np.float64), shift[None, :, None, None].astype(np.float64)
    for _ in range(20):
        bad = np.abs(raw.astype(np.float64) * sc + sf) < 1e-3
        if not bad.any():
            return raw
        raw[bad] = rnd((raw[bad] + np.sign(raw[bad] + 1e-9) * 0.02 + 0.01).astype(np.float32))
    raise AssertionError("could not draw raw away from the mask edge")


class Operands:
    """The two operand sets of one case and their float64 references, computed once and shared by the view loop."""

    def __init__(self, index):
        self.index = index
        self.tag, self.case = TAGGED[index]
        tr, ci, co, k, s, p, op, n, h, w = self.case
        self.T = S.terms(self.case)
        # (a) counting operands
        self.cx, self.cwf = S.counting_inputs(self.case, index, 0)
        self.cdy, self.cwb, self.craw, self.cpw = S.counting_inputs(self.case, index, 1)
        self.cy, self.cdx = S.counting_reference(self.case, 0, self.T), S.counting_reference(self.case, 1, self.T)
        # (b) the sweep's operands, no bias
        self.x, self.w, _, self.dy, self.pw = S.make_inputs(self.case, index, False)
        self._raw, self._f, self._d = {}, {}, {}

    def raw(self, bf16):
        if bf16 not in self._raw:
            rng = np.random.Generator(np.random.PCG64([47, self.index]))
            tr, ci, co, k, s, p, op, n, h, w = self.case
            self._raw[bf16] = _draw_raw(rng, (n, ci, h, w), self.pw[0], self.pw[1], bf16)
        return self._raw[bf16]

    def fwd(self, bf16, in_bf):
        """(x as the view holds it, y reference, bound) of the forward with the sweep's operands."""
        key = (bf16, in_bf)
        if key not in self._f:
            x = S.bf16_round(self.x) if in_bf else self.x
            xa = S.activated(x, self.pw, S.bf16_round if bf16 else None)
            w = (S.bf16_round(self.w) if bf16 else self.w).astype(np.float64)
            self._f[key] = (x, _conv_fwd(self.case, xa, w), _conv_fwd(self.case, np.abs(xa), np.abs(w)))
        return self._f[key]

    def dgrad(self, bf16, in_bf):
        key = (bf16, in_bf)
        if key not in self._d:
            dy = S.bf16_round(self.dy) if in_bf else self.dy
            d64 = (S.bf16_round(dy) if bf16 else dy).astype(np.float64)
            w = (S.bf16_round(self.w) if bf16 else self.w).astype(np.float64)
            self._d[key] = (dy, _conv_dgrad(self.case, d64, w), _conv_dgrad(self.case, np.abs(d64), np.abs(w)))
        return self._d[key]


# -------------------------------------------------------------------------------------------------------- device side
class Ctx:
    def __init__(self, lib, ops_, cid, fails):
        self.lib, self.o, self.cid, self.fails = lib, ops_, cid, fails
        self.case = ops_.case
        self.cv = L.Conv(*self.case[:7])
        self.st = G.stream()
        self.kid = [lib.bp_conv_kernel_id(C.byref(self.cv), d) for d in (L.PACK_FWD, L.PACK_BWD)]
        self.fam = [S.family(i) for i in self.kid]
        self._packed = {}

    def packed(self, which, d, bf16):
        """Packed image of the counting ("c") / sweep ("s") weights for direction d, or None where there is no kernel."""
        key = (which, d, bf16)
        if key not in self._packed:
            lib, cv = self.lib, self.cv
            wt = {("c", 0): self.o.cwf, ("c", 1): self.o.cwb}.get((which, d), self.o.w)
            wd = G.dev(wt)
            if bf16:
                ne = lib.bp_conv_bf16_packed_elems(C.byref(cv), d)
                pk = torch.zeros(ne, device="cuda", dtype=torch.bfloat16) if ne > 0 else None
                if pk is not None:
                    L.check(lib.bp_conv_bf16_pack(C.byref(cv), d, L.ptr(wd), L.ptr(pk), self.st), "bp_conv_bf16_pack")
            else:
                nf = lib.bp_conv_packed_floats(C.byref(cv), d)
                pk = torch.zeros(nf, device="cuda") if nf > 0 else None
                if pk is not None:
                    L.check(lib.bp_conv_pack(C.byref(cv), d, L.ptr(wd), L.ptr(pk), self.st), "bp_conv_pack")
            self._packed[key] = (pk, wd)
        return self._packed[key]


def _poisoned(nsums, nbytes):
    sums = torch.full((nsums + 4,), NAN, dtype=torch.float64, device="cuda")
    ws = torch.full((nbytes // 8 + 8,), NAN, dtype=torch.float64, device="cuda")
    return sums, ws


def _all_nan(*ts):
    return all(torch.isnan(t).all().item() for t in ts)


def _contract(cx, entry, what, call, nb, buf, nsums, check_short):
    """The return-code contract of one call.  `call(sums, ws, bytes)` -> rc.  Returns (sums as numpy, or None)."""
    fails = cx.fails
    sums, ws = _poisoned(nsums, nb)
    if nb == 0:
        rc = call(sums, ws, 64)
        OUTCOMES[entry][rc] += 1
        fails.check(rc == L.BP_EUNSUPPORTED, "%s: no workspace, but return code %d" % (what, rc))
        fails.check(_all_nan(buf, sums), "%s: refused (%d), but the destination or sums were written" % (what, rc))
        return None
    if check_short:
        rc = call(sums, ws, nb - 8)
        fails.check(rc == L.BP_EWORKSPACE, "%s: workspace of %d - 8 bytes: return code %d" % (what, nb, rc))
        fails.check(_all_nan(buf, sums, ws), "%s: workspace too small (%d), but something was written" % (what, rc))
        if rc == L.BP_OK:                                      # (what it wrote must not pass for the real call's)
            buf.fill_(NAN)
            sums.fill_(NAN)
            ws.fill_(NAN)
    rc = call(sums, ws, nb)
    OUTCOMES[entry][rc] += 1
    if rc != L.BP_OK:
        fails.append("%s: a workspace of %d bytes was asked for, but the call returned %d (%s)"
                     % (what, nb, rc, cx.lib.bp_strerror(rc).decode()))
        return None
    s = sums.cpu().numpy()
    fails.check(np.isnan(s[nsums:]).all(), "%s: stores behind the sums" % what)
    fails.check(torch.isnan(ws[nb // 8:]).all().item(), "%s: stores behind the workspace" % what)
    fails.check(not np.isnan(s[:nsums]).any(), "%s: %d elements of the sums were never written" % (what, np.isnan(s[:nsums]).sum()))
    return s[:nsums]


def _worst(key, ratio, cid, what):
    if ratio > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (float(ratio), cid + " [" + what + "]")


def _exact(cx, what, got, want, sums, refs, q_units):
    """(a): bit for bit, exactly -- where every accumulation is exact."""
    EXACT["ok"] += 1
    if max(float(np.max(q)) for q in q_units) >= TWO24:
        EXACT["skipped"] += 1
        return
    EXACT["made"] += 1
    cx.fails.check(np.array_equal(got, want), "%s: %d stored elements differ from the exact result (first at %s)"
                   % (what, (got != want).sum(), np.argwhere(got != want)[:1].tolist()))
    nc = len(refs[0])
    for q, ref in enumerate(refs):
        g = sums[q * nc:(q + 1) * nc]
        cx.fails.check(np.array_equal(g, ref), "%s: sum %d is not exact: channels %s, got - want %s"
                       % (what, q, np.flatnonzero(g != ref)[:6].tolist(), (g - ref)[g != ref][:6].tolist()))


def _within(cx, entry, what, sums, refs, mags, rel, extra=None):
    """(b): |sum - float64 sum of the stored tensor| <= rel * sum|term| (+ extra, an absolute term per sum and channel)."""
    nc = len(refs[0])
    for q, (ref, mag) in enumerate(zip(refs, mags)):
        lim = rel * mag + (extra[q] if extra is not None else 0.0)
        err = np.abs(sums[q * nc:(q + 1) * nc] - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0)).max()
        _worst((entry, "%.3g" % rel), ratio, cx.cid, what)
        cx.fails.check(ratio <= 1.0, "%s: sum %d misses the float64 sum of the stored tensor by %.3g of its limit %.3g sum|term|"
                       % (what, q, ratio, rel))


def _rel_limit(cx, d, bf16):
    if bf16:
        return LIMIT_BF16
    f = fp32_run(cx.fam[d], cx.case)
    return LIMIT_DOUBLE + f * U32


def _forward(cx, which, kind, impl_bf16, in_bf, out_bf, bn):
    lib, o, cv, st, fails = cx.lib, cx.o, cx.cv, cx.st, cx.fails
    tr, ci, co, k, s, p, op, n, h, w = cx.case
    ho, wo = S.out_shape(cx.case)
    entry = "forward_stats bf16" if impl_bf16 else "forward_stats"
    where = "%s %s %s-%s" % (which, kind, "bf16" if in_bf else "f32", "bf16" if out_bf else "f32")
    what = "%s [%s]" % (entry, where)
    pk, wd = cx.packed(which, 0, impl_bf16)
    impl = L.IMPL_BF16 if impl_bf16 else L.IMPL_MFMA
    if which == "c":
        x_in, keep, pwp = o.cx, None, None
    else:
        x_in, y_ref, y_bnd = o.fwd(impl_bf16, in_bf)
        keep, pw = G.pointwise(*o.pw)
        pwp = C.byref(pw)
    xb, xv = _in_view(x_in, kind, in_bf)
    yb, yv = _out_view(n, co, ho, wo, kind, out_bf)
    nb = lib.bp_conv_stats_workspace(C.byref(cv), L.PACK_FWD, C.byref(xv), C.byref(yv), impl)
    if pk is None:
        fails.check(nb == 0, "%s: a workspace of %d bytes for a direction without a packed image" % (what, nb))
        OUTCOMES[entry]["no image"] += 1
        return

    def call(sums, ws, nbytes):
        return lib.bp_conv_forward_stats(C.byref(cv), C.byref(xv), pwp, L.ptr(pk), C.byref(yv), L.ptr(sums), L.ptr(ws), nbytes, impl, st)

    sums = _contract(cx, entry, what, call, nb, yb, 2 * co, which == "c")
    if sums is None:
        return
    got, clean = _read(yb, yv)
    fails.check(clean, "%s: stores outside the view" % what)
    if not impl_bf16 and kind == "aligned":
        SERVED[(0, cx.fam[0])] += 1
    if not impl_bf16 and cx.fam[0] in TILED:
        rows = S.stats_rows(nb, co)
        if rows is not None:
            REGIMES[(0, S.fold_regime(rows))] += 1
    if not np.isfinite(got).all():
        fails.append("%s: non-finite values inside the view" % what)
        return
    if which == "c":
        refs, mags, _ = S.stats_reference(1, o.cy)
        _exact(cx, what, got, o.cy, sums, refs, [mags[1]])
        return
    _judge(fails, cx.cid, "bf16/stats" if impl_bf16 else "mfma/stats", "y", got, y_ref, y_bnd, o.T[0], out_bf, "stats " + where)
    refs, mags, _ = S.stats_reference(1, got)
    _within(cx, entry, what, sums, refs, mags, _rel_limit(cx, 0, impl_bf16))
    if bn:
        _forward_bn(cx, what, xv, pwp, pk, yb, sums, nb, kind)


def _forward_bn(cx, what, xv, pwp, pk, yb_stats, sums_stats, nb, kind):
    """bp_conv_forward_bn == bp_conv_forward_stats followed by bp_bn_finalize, bit for bit (the nine outputs)."""
    lib, cv, st = cx.lib, cx.cv, cx.st
    tr, ci, co, k, s, p, op, n, h, w = cx.case
    ho, wo = S.out_shape(cx.case)
    rng = np.random.Generator(np.random.PCG64([53, cx.o.index]))
    gamma, beta = G.dev(rng.uniform(0.5, 1.5, co).astype(np.float32)), G.dev(rng.uniform(-0.5, 0.5, co).astype(np.float32))
    cnt = float(n * ho * wo)
    out = []
    for fused in (False, True):
        rm, rv = torch.full((co,), 0.25, device="cuda"), torch.full((co,), 0.75, device="cuda")
        nbt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        scale, shift = torch.full((co,), NAN, device="cuda"), torch.full((co,), NAN, device="cuda")
        sm, si = torch.full((co,), NAN, dtype=torch.float64, device="cuda"), torch.full((co,), NAN, dtype=torch.float64, device="cuda")
        if fused:
            yb, yv = _out_view(n, co, ho, wo, kind)
            sums = torch.full((3 * co,), NAN, dtype=torch.float64, device="cuda")
            ws = torch.full((nb // 8 + 8,), NAN, dtype=torch.float64, device="cuda")
            bt = L.BnTrain(cnt, gamma.data_ptr(), beta.data_ptr(), 1e-5, 0.1, rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(),
                           scale.data_ptr(), shift.data_ptr(), sm.data_ptr(), si.data_ptr())
            rc = lib.bp_conv_forward_bn(C.byref(cv), C.byref(xv), pwp, L.ptr(pk), C.byref(yv), L.ptr(sums), C.byref(bt),
                                        L.ptr(ws), nb, L.IMPL_MFMA, st)
            OUTCOMES["forward_bn"][rc] += 1
            if rc != L.BP_OK:
                cx.fails.append("%s: bp_conv_forward_bn returned %d where bp_conv_forward_stats returned BP_OK" % (what, rc))
                return
            ysame = torch.equal(torch.nan_to_num(yb, nan=-7.0), torch.nan_to_num(yb_stats, nan=-7.0))
            s2 = sums[:2 * co].cpu().numpy()
        else:
            sums = torch.from_numpy(np.concatenate([sums_stats, np.full(co, NAN)])).cuda()
            L.check(lib.bp_bn_finalize(L.ptr(sums), cnt, co, L.ptr(gamma), L.ptr(beta), 1e-5, 0.1, L.ptr(rm), L.ptr(rv),
                                       L.ptr(nbt), L.ptr(scale), L.ptr(shift), L.ptr(sm), L.ptr(si), st))
            ysame, s2 = True, sums_stats
        out.append([ysame, s2] + [t.cpu().numpy() for t in (scale, shift, sm, si, rm, rv, nbt)])
    BN_COMPARED[0] += 1
    names = ("y", "sums", "scale", "shift", "save_mean", "save_invstd", "running_mean", "running_var", "num_batches_tracked")
    cx.fails.check(out[1][0] is True, "%s: bp_conv_forward_bn stored another y" % what)
    for name, a, b in list(zip(names, *out))[1:]:
        cx.fails.check(np.array_equal(a, b), "%s: bp_conv_forward_bn differs from stats + finalize in %s" % (what, name))
    cx.fails.check(out[1][8][0] == 8, "%s: the batch counter" % what)


def _dgrad(cx, which, kind, raw_kind, bf16, dy_bf):
    """bp_conv_backward_data_stats.  bf16: dx and raw bf16 views (the bf16 kernels), dy bf16 or fp32."""
    lib, o, cv, st, fails = cx.lib, cx.o, cx.cv, cx.st, cx.fails
    tr, ci, co, k, s, p, op, n, h, w = cx.case
    entry = "backward_data_stats bf16" if bf16 else "backward_data_stats"
    where = "%s %s raw-%s%s" % (which, kind, raw_kind, (" dy-bf16" if dy_bf else " dy-f32") if bf16 else "")
    what = "%s [%s]" % (entry, where)
    pk, wd = cx.packed(which, 1, bf16)
    if which == "c":
        dy_in, raw, pwv = o.cdy, o.craw, o.cpw
    else:
        dy_in, dx_ref, dx_bnd = o.dgrad(bf16, dy_bf)
        raw, pwv = o.raw(bf16), o.pw
    keep, pw = G.pointwise(*pwv)
    dyb, dyv = _in_view(dy_in, kind, dy_bf)
    rb, rv = _in_view(raw, raw_kind, bf16)
    dxb, dxv = _out_view(n, ci, h, w, kind, bf16)
    nb = lib.bp_conv_stats_workspace(C.byref(cv), L.PACK_BWD, C.byref(dxv), C.byref(dyv), L.IMPL_BF16 if bf16 else L.IMPL_MFMA)
    if pk is None:
        fails.check(nb == 0, "%s: a workspace of %d bytes for a direction without a packed image" % (what, nb))
        OUTCOMES[entry]["no image"] += 1
        return

    def call(sums, ws, nbytes):
        return lib.bp_conv_backward_data_stats(C.byref(cv), C.byref(dyv), L.ptr(pk), C.byref(dxv), C.byref(rv), C.byref(pw),
                                               L.ptr(sums), L.ptr(ws), nbytes, st)

    sums = _contract(cx, entry, what, call, nb, dxb, 2 * ci, which == "c")
    if sums is None:
        return
    got, clean = _read(dxb, dxv)
    fails.check(clean, "%s: stores outside the view" % what)
    if not bf16 and kind == "aligned" and raw_kind == "aligned":
        SERVED[(1, cx.fam[1])] += 1
    if not bf16 and cx.fam[1] in TILED:
        rows = S.stats_rows(nb, ci)
        if rows is not None:
            REGIMES[(1, S.fold_regime(rows))] += 1
    if not np.isfinite(got).all():
        fails.append("%s: non-finite values inside the view" % what)
        return
    if which == "c":
        refs, mags, _ = S.stats_reference(2, o.cdx, raw, pwv)
        _exact(cx, what, got, o.cdx, sums, refs, [4 * mags[1]])
        return
    _judge(fails, cx.cid, "bf16/stats" if bf16 else "mfma/stats", "dx", got, dx_ref, dx_bnd, o.T[1], bf16, "stats " + where)
    refs, mags, _ = S.stats_reference(2, got, raw, pwv)
    _within(cx, entry, what, sums, refs, mags, _rel_limit(cx, 1, bf16))


def _act(cx, which, kind, bf16):
    """bp_conv_backward_data_act: g stored in place of dx and the three sums.  bf16: g and raw bf16, dy fp32 (the head kernel)."""
    lib, o, cv, st, fails = cx.lib, cx.o, cx.cv, cx.st, cx.fails
    tr, ci, co, k, s, p, op, n, h, w = cx.case
    entry = "backward_data_act bf16" if bf16 else "backward_data_act"
    where = "%s %s" % (which, kind)
    what = "%s [%s]" % (entry, where)
    pk, wd = cx.packed(which, 1, bf16)
    if which == "c":
        dy_in, raw, pwv = o.cdy, o.craw, o.cpw
    else:
        dy_in, dx_ref, dx_bnd = o.dgrad(bf16, False)
        raw, pwv = o.raw(bf16), o.pw
    keep, pw = G.pointwise(*pwv)
    dyb, dyv = _in_view(dy_in, kind, False)
    rb, rv = _in_view(raw, kind, bf16)
    gb, gv = _out_view(n, ci, h, w, kind, bf16)
    nb = lib.bp_conv_backward_data_act_workspace(C.byref(cv), C.byref(dyv), C.byref(gv))
    if pk is None:
        fails.check(nb == 0, "%s: a workspace of %d bytes for a direction without a packed image" % (what, nb))
        OUTCOMES[entry]["no image"] += 1
        return

    def call(sums, ws, nbytes):
        return lib.bp_conv_backward_data_act(C.byref(cv), C.byref(dyv), L.ptr(pk), C.byref(gv), C.byref(rv), C.byref(pw),
                                             L.ptr(sums), L.ptr(ws), nbytes, st)

    sums = _contract(cx, entry, what, call, nb, gb, 3 * ci, which == "c")
    if sums is None:
        return
    got, clean = _read(gb, gv)
    fails.check(clean, "%s: stores outside the view" % what)
    if not np.isfinite(got).all():
        fails.append("%s: non-finite values inside the view" % what)
        return
    if which == "c":
        refs, mags, g = S.stats_reference(3, o.cdx, raw, pwv)
        _exact(cx, what, got, g, sums, refs, [4 * mags[1], 4 * mags[2]])
        return
    # dx itself, as the same kernel stores it without the epilogue
    dxb, dxv = _out_view(n, ci, h, w, kind, bf16)
    L.check(lib.bp_conv_backward_data(C.byref(cv), C.byref(dyv), L.ptr(pk), L.ptr(wd), C.byref(dxv),
                                      L.IMPL_BF16 if bf16 else L.IMPL_MFMA, st), what + ": bp_conv_backward_data")
    dx, _ = _read(dxb, dxv)
    refs, mags, g = S.stats_reference(3, dx, raw, pwv)
    sc, sf, sl = (np.asarray(v, np.float64)[None, :, None, None] for v in pwv)
    t32 = (np.asarray(raw, np.float64) * sc + sf).astype(np.float32)
    g_ref = np.where(t32 > 0, dx_ref, dx_ref * sl)
    _judge(fails, cx.cid, "bf16/stats" if bf16 else "mfma/stats", "dx", got, g_ref, dx_bnd, o.T[1], bf16, "act " + where)
    if not bf16:
        fails.check(np.array_equal(got, g), "%s: g is not dx or the fp32 product dx * slope of the dx the kernel stores" % what)
        _within(cx, entry, what, sums, refs, mags, _rel_limit(cx, 1, False))
        return
    # the kernel sums the unrounded gradient, the reference the stored bf16 one: half a bf16 ulp of every term
    hu = np.ldexp(1.0, np.frexp(np.abs(dx))[1] - 9) * (dx != 0)
    extra = [f.sum(axis=(0, 2, 3)) for f in (hu, hu * np.abs(raw.astype(np.float64)), hu * np.abs(t32.astype(np.float64)))]
    _within(cx, entry, what, sums, refs, mags, LIMIT_BF16, extra)


def _run_all(cx):
    lib, cv = cx.lib, cx.cv
    bf = [lib.bp_conv_bf16_supported(C.byref(cv), d, None, None) == 1 for d in (L.PACK_FWD, L.PACK_BWD)]
    for which in ("c", "s"):
        for kind in ("aligned", "odd"):
            _forward(cx, which, kind, False, False, False, bn=which == "s" and kind == "aligned")
            _dgrad(cx, which, kind, kind, False, False)
            if kind == "aligned":
                _dgrad(cx, which, kind, "odd", False, False)
            _act(cx, which, kind, False)
            if bf[0]:
                _forward(cx, which, kind, True, True, True, False)
                _forward(cx, which, kind, True, False, False, False)
            if bf[1]:
                _dgrad(cx, which, kind, kind, True, True)
                if kind == "aligned":
                    _dgrad(cx, which, kind, kind, True, False)
                _act(cx, which, kind, True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("index", range(len(TAGGED)), ids=[S.case_id(t, c) for t, c in TAGGED])
def test_statistics_sweep(index):
    lib = L.load()
    o = Operands(index)
    cid = S.case_id(*TAGGED[index])
    fails = Failures()
    switches = SWITCHES.get(tuple(o.case[:7]), ())
    try:
        for setting in ((1, 0) if switches else (None,)):
            for name in switches:
                assert lib.bp_set_option(name, setting) == 0
            before = len(fails)
            _run_all(Ctx(lib, o, cid, fails))
            if switches:
                fails[before:] = ["[%s = %d] %s" % (b", ".join(switches).decode(), setting, f) for f in fails[before:]]
    finally:
        for name in switches:
            lib.bp_set_option(name, -1)
    RAN.add(index)
    assert not fails, "%s: %d failures\n  " % (cid, len(fails)) + "\n  ".join(fails[:40])


def test_statistics_sweep_report():
    """Calls per outcome per entry point, the worst ratio to each limit with its case, the exact checks made and skipped,
    over the cases that ran in this process (-s).  When the whole file ran: at most 5 % of the BP_OK calls with counting
    operands skipped the exact check, every family of the CPU table (test_conv_sweep_ref.py STATS_TABLE) served a BP_OK
    call in each direction it has, and the three regimes of the first fold each ran in both directions."""
    print()
    names = {L.BP_OK: "BP_OK", L.BP_EUNSUPPORTED: "BP_EUNSUPPORTED", L.BP_EWORKSPACE: "BP_EWORKSPACE", L.BP_EINVAL: "BP_EINVAL"}
    for entry in sorted(OUTCOMES):
        print("%-26s %s" % (entry, "   ".join("%s %d" % (names.get(k, str(k)), v) for k, v in sorted(OUTCOMES[entry].items(), key=str))))
    for key in sorted(WORST):
        print("worst sums   %-26s limit %-8s %10.3g of the limit   %s" % (key + WORST[key]))
    for key in sorted(k for k in CONV_WORST if k[1].endswith("/stats")):
        print("worst stored %-12s %-10s %-3s %8.3f of the limit   %s" % (key + CONV_WORST[key]))
    print("exact checks: %d made, %d skipped (Q >= 2^24) of %d BP_OK calls with counting operands; bp_conv_forward_bn compared %d times"
          % (EXACT["made"], EXACT["skipped"], EXACT["ok"], BN_COMPARED[0]))
    print("served (direction, family): " + ", ".join("%d/%s %d" % (k + (v,)) for k, v in sorted(SERVED.items())))
    print("fold regimes of the tiled kernels (direction, regime): " + ", ".join("%d/%s %d" % (k + (v,)) for k, v in sorted(REGIMES.items())))
    print("%d of %d cases ran in this process" % (len(RAN), len(TAGGED)))
    if len(RAN) == len(TAGGED):
        assert EXACT["skipped"] <= 0.05 * EXACT["ok"], EXACT
        assert EXACT["made"] > 0 and BN_COMPARED[0] > 0
        for d, fams in ((0, FWD_FAMILIES), (1, BWD_FAMILIES)):
            for f in fams:
                assert SERVED[(d, f)] > 0, "no BP_OK call served by family %s in direction %d" % (f, d)
            for regime in ("direct", "fold32", "fold256"):
                assert REGIMES[(d, regime)] > 0, "fold regime %s never ran in direction %d" % (regime, d)
