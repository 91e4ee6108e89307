"""GPU: the persistent forward / data-gradient kernels where every workgroup walks three and four tiles
(tests/walk_sweep.py; test_walk_sweep_host.py pins which kernel serves each case and how deep it walks).

tests/test_gpu_conv_sweep.py draws tensors of at most 3 x 22 x 40 and test_gpu_stats_sweep.py adds walks of two tiles for
2 workgroups of some kernels, through the statistics entry points: the steady state of the fetch / commit pipeline, a
clipped tile followed by a full one in the same walk, and walks that cross images with a ragged remainder were run by no
test.  The cases here reach them by extent alone, in the production configuration (no environment switch, no subprocess),
through plain bp_conv_forward / bp_conv_backward_data.

Per case: BP_IMPL_MFMA and BP_IMPL_AUTO on a 16-byte addressable channel slice of a wider buffer and on a slice with odd
stride and offset (conv_sweep_gpu._in_view / _out_view: the two pick the OUT_VEC / in_vec instantiations), and, for the
four families that store 16 bytes at a time and refuse an odd produced view under BP_IMPL_MFMA (BP_IMPL_AUTO takes the
direct kernel there), the odd gathered view with the aligned produced one, so that their scalar-load staging walks too.
BP_IMPL_BF16 wherever bp_conv_bf16_supported accepts the aligned views: bf16 on both sides for the fp32 cases, all four
pairs of element types for the cases listed for the persistent bf16 kernel (with bf16 on both sides and extents in the
ratio 2 the flattened-K bf16 kernels take the 16 <-> 32 k4 s2 layers; the other three pairs reach the persistent one).
Outputs are pre-filled with NaN; after BP_OK every channel outside the view is still NaN, after a refusal everything is.

Every result is judged twice:
  a. exactly: operands drawn per element from -2 .. 2 (weights -1 .. 1), a pending activation with scale 1, shift in
     {0, 1} and slope in {0, 1/2, 1} on the forward cases and an integer bias on every other one -- every product and
     partial sum is an integer or half-integer below 2^23, exact in any order, so the stored tensor equals the float64
     reference, no tolerance (a bf16 result: its rounding to bf16).  A pixel from the wrong tile or image changes it;
  b. conv_sweep.make_inputs operands through conv_sweep_gpu._judge: the convolution sweep's two criteria and limits.

No case failed on its first run on the GPU: no kernel had to be fixed, and walk_sweep.REGRESSIONS is empty.  Calls by
return code (28 cases, both passes): BP_IMPL_MFMA 112 BP_OK and 20 BP_EUNSUPPORTED -- the odd produced views of flat_h7,
flat_t4, flat_t64 and flat_g4, 10 cases x 2 passes, each with the destination still all NaN --, BP_IMPL_AUTO 112 BP_OK,
BP_IMPL_BF16 112 BP_OK; no exact check was skipped.  Worst ratios to the limits of _judge: BP_IMPL_MFMA 0.050 (max-relative)
and 0.339 (elementwise), BP_IMPL_AUTO 0.069 and 0.339, BP_IMPL_BF16 0.857 and 1.000 (a bf16 result half an ulp from the
reference).

That the sweep notices was checked once with two kernels of conv_flat.hip made wrong on purpose, in the numbers only:
flat_k7_kernel fetching tile t + 2 grid where the walk has one (so a workgroup's second tile is its third; walks of two
tiles are unchanged) and flat_t4_kernel keeping the bits of the previous tile's mask (inside |= in).  The four cases of
those kernels and the two bf16 cases whose fp32 runs they serve failed both criteria (flat_k7: 1990401 of 6000048
elements differ, the first in image 56 = tile 512, by up to 132; flat_t4: 159735 of 6139584, by up to 47.5; _judge
1.2e5 of the elementwise limit); the other 22 cases passed, and so did every flat_k7 and flat_t4 case (gates, neighbours)
of test_gpu_conv_sweep.py and test_gpu_stats_sweep.py and every walk:* case of the latter, walk:f:flat_t4 among them.

Wall time on one MI355X, both measured in one visit: this file 30 s (28 cases and the report; the slowest case, the stem
with its 96 MB output, 4.3 s), tests/test_gpu_conv_sweep.py 61 s.  Every n is already the smallest its walk allows.
"""
import collections
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import conv_sweep as S
import gpu_util as G
import walk_sweep as W
from conv_sweep_gpu import WORST, Failures, _in_view, _judge, _out_view, _read

pytestmark = pytest.mark.gpu
W.require_production_environment()

# seconds of `pytest -m gpu` for this file / for tests/test_gpu_conv_sweep.py, measured in the same visit on one MI355X
WALL_TIME = {"test_gpu_walk_sweep.py": 30, "test_gpu_conv_sweep.py": 61}

IMPLS = {"mfma": L.IMPL_MFMA, "auto": L.IMPL_AUTO, "bf16": L.IMPL_BF16}
# kernel ids of the families that refuse a produced view they cannot store 16 bytes at a time (BP_IMPL_MFMA only)
VEC_OUT_IDS = {r.kid for r in W.INST.values() if r.vec_out}

OUTCOMES = collections.defaultdict(collections.Counter)       # impl -> {return code: calls}
SECONDS = {}                                                  # case id -> wall time of its test
RAN = set()


def _stop_on_fault(test):
    """Chain nothing after a failure of the device: a HIP error in one case ends the run, the cases after it do not
    launch on a device in that state."""
    @functools.wraps(test)
    def wrapped(*args, **kwargs):
        try:
            return test(*args, **kwargs)
        except RuntimeError as ex:
            if "HIP error" in str(ex) or "hipError" in str(ex):
                pytest.exit("device error, nothing more is launched: %s" % str(ex).splitlines()[0], returncode=3)
            raise
    return wrapped


class Host:
    """Operands and float64 results of one case, computed once and shared by the impl x view loop."""

    def __init__(self, index):
        self.e = e = W.ENTRIES[index]
        fwd = e.direction == W.FWD
        self.g, self.w, self.bias, self.pw = W.exact_inputs(e, index)
        self.ref = W.reference(e.case, e.direction, self.g, self.w, self.bias, self.pw)
        self.ref_nobias = self.ref if self.bias is None else W.reference(e.case, e.direction, self.g, self.w, None, self.pw)
        x, self.wr, bias, dy, pw = S.make_inputs(e.case, 5000 + index, fwd and index % 2 == 0)
        self.gr, self.biasr, self.pwr = (x, bias, pw) if fwd else (dy, None, None)
        self.T = W.terms(e.case, e.direction)
        self._f32, self._bf = {}, {}

    def f32(self, biased):
        if biased not in self._f32:
            a = (self.e.case, self.e.direction, self.gr, self.wr, self.biasr if biased else None, self.pwr)
            self._f32[biased] = (W.reference(*a), W.bound(*a))
        return self._f32[biased]

    def bf16(self, in_bf):
        """Against the bf16-rounded operands: bf16 views hold rounded tensors, the kernel rounds what it stages."""
        if in_bf not in self._bf:
            g = S.bf16_round(self.gr) if in_bf else self.gr
            a = (self.e.case, self.e.direction, g, S.bf16_round(self.wr), None, self.pwr, S.bf16_round)
            self._bf[in_bf] = (W.reference(*a), W.bound(*a))
        return self._bf[in_bf]


class Device:
    """Device copies of one case's operands: views made on demand, packed images per implementation."""

    def __init__(self, lib, host, cv):
        self.lib, self.host, self.cv, self._v, self._p = lib, host, cv, {}, {}
        self.w = {"exact": G.dev(host.w), "random": G.dev(host.wr)}
        self.bias = {"exact": G.dev(host.bias) if host.bias is not None else None,
                     "random": G.dev(host.biasr) if host.biasr is not None else None}
        self.pw = {"exact": G.pointwise(*host.pw) if host.pw is not None else (None, None),
                   "random": G.pointwise(*host.pwr) if host.pwr is not None else (None, None)}

    def gathered(self, which, kind, bf):
        key = (which, kind, bf)
        if key not in self._v:
            a = self.host.g if which == "exact" else self.host.gr
            self._v[key] = _in_view(S.bf16_round(a) if bf else a, kind, bf)
        return self._v[key][1]

    def packed(self, which, bf):
        key = (which, bf)
        if key not in self._p:
            d, st, pcv = self.host.e.direction, G.stream(), C.byref(self.cv)
            if bf:
                pk = torch.zeros(self.lib.bp_conv_bf16_packed_elems(pcv, d), device="cuda", dtype=torch.bfloat16)
                rc = self.lib.bp_conv_bf16_pack(pcv, d, L.ptr(self.w[which]), L.ptr(pk), st)
            else:
                pk = torch.zeros(self.lib.bp_conv_packed_floats(pcv, d), device="cuda")
                rc = self.lib.bp_conv_pack(pcv, d, L.ptr(self.w[which]), L.ptr(pk), st)
            assert rc == L.BP_OK, "pack: %d" % rc
            self._p[key] = pk
        return self._p[key]

    def call(self, which, impl, gv, pv, biased):
        e, pcv, st = self.host.e, C.byref(self.cv), G.stream()
        bf = impl == "bf16"
        pk, wd = self.packed(which, bf), self.w[which]
        if e.direction == W.BWD:
            return self.lib.bp_conv_backward_data(pcv, C.byref(gv), L.ptr(pk), L.ptr(wd), C.byref(pv), IMPLS[impl], st)
        pw = self.pw[which][1]
        return self.lib.bp_conv_forward(pcv, C.byref(gv), C.byref(pw) if pw is not None else None, L.ptr(pk), L.ptr(wd),
                                        L.ptr(self.bias[which]) if biased else None, C.byref(pv), IMPLS[impl], st)


def _runs(lib, e, cv, kid):
    """[(impl, kind of the gathered view, kind of the produced view, gathered bf16, produced bf16, may refuse)]"""
    pairs = [("aligned", "aligned"), ("odd", "odd")] + ([("odd", "aligned")] if kid in VEC_OUT_IDS else [])
    out = [(impl, ik, ok, False, False, impl == "mfma" and ok == "odd" and kid in VEC_OUT_IDS)
           for impl in ("mfma", "auto") for ik, ok in pairs if impl == "mfma" or ik == ok]
    gs, ps = W.operand_shapes(e.case, e.direction)
    for ib, ob in ((True, True), (False, False), (False, True), (True, False)) if e.impl == "bf16" else ((True, True),):
        gv, pv = _out_view(1, gs[1], 1, 1, "aligned", ib)[1], _out_view(1, ps[1], 1, 1, "aligned", ob)[1]
        if lib.bp_conv_bf16_supported(C.byref(cv), e.direction, C.byref(gv), C.byref(pv)) == 1:
            out.append(("bf16", "aligned", "aligned", ib, ob, False))
    return out


def _exact(fails, what, buf, view, want_nchw):
    """The stored view against the float64 reference of the integer data, compared on the device: every element equal,
    every channel outside the view still NaN."""
    want = torch.from_numpy(np.ascontiguousarray(want_nchw.transpose(0, 2, 3, 1))).cuda()
    f = buf.to(torch.float64)
    inside = f[..., view.coff:view.coff + view.c]
    bad = inside != want                                       # (NaN differs from everything)
    nbad = int(bad.sum())
    if nbad:
        diff = (inside - want)[bad].abs()
        n, y, x, c = (int(v[0]) for v in torch.nonzero(bad)[:1].unbind(1))
        fails.append("%s: %d of %d elements differ from the float64 reference of the integer data (largest difference %s; "
                     "first at image %d, pixel (%d, %d), channel %d)" % (what, nbad, want.numel(), float(diff.max()), n, y, x, c))
    clean = torch.isnan(f[..., :view.coff]).all().item() and torch.isnan(f[..., view.coff + view.c:]).all().item()
    fails.check(clean, "%s: stores outside the view" % what)


@pytest.mark.parametrize("index", range(len(W.ENTRIES)), ids=[W.case_id(e) for e in W.ENTRIES])
@_stop_on_fault
def test_walk_sweep(index):
    t0 = time.perf_counter()
    lib = L.load()
    e = W.ENTRIES[index]
    cid = W.case_id(e)
    cv = L.Conv(*e.case[:7])
    kid = lib.bp_conv_kernel_id(C.byref(cv), e.direction)
    assert W.exact_magnitude(e) < W.EXACT_LIMIT
    host = Host(index)
    dev = Device(lib, host, cv)
    _, (n, pc, ph, pwd) = W.operand_shapes(e.case, e.direction)
    fails = Failures()
    listed = 0
    for impl, ik, ok, ib, ob, refuses in _runs(lib, e, cv, kid):
        where = "%s>%s %s>%s" % (ik, ok, "bf16" if ib else "f32", "bf16" if ob else "f32")
        b16 = impl == "bf16"
        for which in ("exact", "random"):
            what = "%s %s [%s] %s" % (cid, impl, where, which)
            biased = not b16 and (host.bias if which == "exact" else host.biasr) is not None
            gv = dev.gathered(which, ik, ib)
            buf, pv = _out_view(n, pc, ph, pwd, ok, ob)
            rc = dev.call(which, impl, gv, pv, biased)
            OUTCOMES[impl][rc] += 1
            if refuses:
                fails.check(rc == L.BP_EUNSUPPORTED and torch.isnan(buf).all().item(),
                            "%s: returned %d for a produced view the kernel cannot store to (or wrote to it)" % (what, rc))
                continue
            if rc != L.BP_OK:
                fails.append("%s: return code %d (%s)" % (what, rc, lib.bp_strerror(rc).decode()))
                continue
            listed += impl == e.impl and ik == "aligned"
            if which == "exact":
                ref = host.ref if biased else host.ref_nobias
                _exact(fails, what, buf, pv, S.bf16_round(ref.astype(np.float32)).astype(np.float64) if ob else ref)
            else:
                ref, bnd = host.bf16(ib) if b16 else host.f32(biased)
                got, clean = _read(buf, pv)
                fails.check(clean, "%s: stores outside the view" % what)
                _judge(fails, cid, impl, "y" if e.direction == W.FWD else "dx", got, ref, bnd, host.T, ob, where)
    torch.cuda.synchronize()
    assert listed, "%s: the run the case is listed for did not happen" % cid
    RAN.add(index)
    SECONDS[cid] = time.perf_counter() - t0
    assert not fails, "%s: %d failures\n  " % (cid, len(fails)) + "\n  ".join(fails[:40])


def test_walk_sweep_report():
    """Outcomes per implementation, the worst ratio to each limit of conv_sweep_gpu._judge and the slowest cases over what
    ran in this process (-s).  A report: under -k it covers the selected cases only.  When the whole file ran, every call
    returned BP_OK except BP_IMPL_MFMA on the odd produced views of the four families that store 16 bytes at a time."""
    print()
    for impl in IMPLS:
        oc = OUTCOMES[impl]
        other = sum(v for k, v in oc.items() if k not in (L.BP_OK, L.BP_EUNSUPPORTED))
        print("%-6s BP_OK %6d   BP_EUNSUPPORTED %6d   other %d" % (impl, oc[L.BP_OK], oc[L.BP_EUNSUPPORTED], other))
    for key in sorted(WORST):
        print("worst %-12s %-6s %-5s %8.3f of the limit   %s" % (key + WORST[key]))
    for cid in sorted(SECONDS, key=SECONDS.get, reverse=True)[:5]:
        print("%6.1f s  %s" % (SECONDS[cid], cid))
    print("%d of %d cases ran in this process, %.1f s in all" % (len(RAN), len(W.ENTRIES), sum(SECONDS.values())))
    assert set(OUTCOMES["auto"]) <= {L.BP_OK} and set(OUTCOMES["bf16"]) <= {L.BP_OK}
    assert set(OUTCOMES["mfma"]) <= {L.BP_OK, L.BP_EUNSUPPORTED}
    if len(RAN) == len(W.ENTRIES):
        lib = L.load()
        vec = sum(1 for e in W.ENTRIES if lib.bp_conv_kernel_id(C.byref(L.Conv(*e.case[:7])), e.direction) in VEC_OUT_IDS)
        # per case and pass: the two layouts, and for the vec families the mixed one in place of the refused odd one
        assert OUTCOMES["mfma"][L.BP_EUNSUPPORTED] == 2 * vec
        assert OUTCOMES["mfma"][L.BP_OK] == 4 * len(W.ENTRIES)
        assert OUTCOMES["auto"][L.BP_OK] == 4 * len(W.ENTRIES)
        assert OUTCOMES["bf16"][L.BP_OK] >= 2 * 4 * sum(1 for e in W.ENTRIES if e.impl == "bf16")
