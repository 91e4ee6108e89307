"""GPU: every convolution implementation behind the C ABI, swept over the geometries of tests/conv_sweep.py.

The operator tests run the kernels at the model's own layers.  The dispatcher (igemm_config / bp_igemm_run, b_config,
bp_wgrad_select) picks kernels from the geometry alone, and these paths are reachable through the ABI without being one
of those layers -- the gaps the sweep's targeted cases are numbered after:
  1. the plain igemm_kernel for wide layers (a view that is not 16-byte addressable drops a DMA layer to it);
  2. channel counts off the 4 / 8 / 16 grids: zero-padded chunk tails, the `co < cout` masks, pixel packing COP 4 and 8;
  3. transposed-form tap masks: k % stride != 0, k < stride (phases without a tap), stride 3, k 1, 2, 6;
  4. pad 0, pad >= k, trailing input rows that no output reads, out_pad, tensors below one tile, h = 1, w = 1, 1 x 1;
  5. BP_IMPL_AUTO's fall-back to the direct kernel, and the direct kernels themselves;
  6. everything bp_conv_bf16_supported accepts;
  7. dbias.

Per case: forward with a pending activation whose act(0) != 0 (and a bias on every third case), data gradient, weight
gradient (with dbias on the biased cases), for BP_IMPL_DIRECT, BP_IMPL_MFMA, BP_IMPL_AUTO and -- where
bp_conv_bf16_supported accepts the actual views -- BP_IMPL_BF16 with bf16 and fp32 views on either side; each on a
16-byte addressable channel slice of a wider buffer and on a slice with odd channel stride and offset.  Outputs are
pre-filled with NaN.

Return codes.  BP_OK: the result is judged and every channel outside the view is still NaN.  BP_EUNSUPPORTED
(BP_IMPL_MFMA / BP_IMPL_BF16 only): the destination is still all NaN.  BP_IMPL_DIRECT and BP_IMPL_AUTO return BP_OK on
every case (csrc/conv_direct.hip documents no limit).  BP_IMPL_BF16 returns BP_OK wherever bp_conv_bf16_supported said 1
and the call carries no bias.

Judgement, both criteria:
  1. the suite's limits relative to the tensor's maximum: 2e-5 forward / data gradient, 1e-4 weight gradient, 4e-3 for
     a result stored as bf16; bf16 runs against the float64 convolution of the bf16-rounded operands;
  2. elementwise |got - ref| <= (T + 2) 2^-24 B, T the number of products behind the element and B the sum of their
     magnitudes (+ |bias|): the worst case of a length-T fp32 sum in any order, with one rounding each for the
     activation's slope and the bias; plus half a bf16 ulp where the result is stored as bf16 (taken at |ref| plus the
     fp32 term, which is what was rounded).  Where B = 0 -- phases without a tap, rows no output reads -- the result is
     exactly the bias, or 0.

Wall time on one MI355X, both measured in one visit: this file 60 s (753 cases + the report), tests/test_gpu_ops.py 177 s
(unchanged since the commit before the sweep): a third of it, against a limit of twice; no draw was thinned.  No case met
criterion 1 and missed criterion 2 or the reverse: the worst max-relative ratios are 0.23 (fp32) and 0.94 (bf16 stored) of
their limits, the worst elementwise ones 0.63 (fp32) and 1.00 (a bf16 result half an ulp from the reference).
"""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import conv_sweep as S
import gpu_util as G
from conv_sweep_gpu import TAGGED, WORST, Failures, Host, _in_view, _judge, _out_view, _read

pytestmark = pytest.mark.gpu

# seconds of `pytest -m gpu` for this file / for tests/test_gpu_ops.py, measured in the same visit on one MI355X
WALL_TIME = {"test_gpu_conv_sweep.py": 60, "test_gpu_ops.py": 177}

IMPLS = {"direct": L.IMPL_DIRECT, "mfma": L.IMPL_MFMA, "auto": L.IMPL_AUTO, "bf16": L.IMPL_BF16}

# bp_set_option switches between a special kernel and the tiled one: layers they apply to (both settings are run)
SWITCHES = {
    (0, 128, 128, 3, 1, 1, 0): (b"f32_ws", b"f32_wgrad_ws", b"bf16_ws", b"bf16_wgrad_ws"),
    (0, 64, 128, 4, 2, 1, 0): (b"bf16_ws",),
    (1, 128, 64, 4, 2, 1, 0): (b"bf16_ws",),
}

OUTCOMES = collections.defaultdict(collections.Counter)       # impl -> {return code: calls}
RAN = set()                                                   # indices of the cases that ran in this process


def _outcome(fails, impl, rc, what, buf, view, may_refuse):
    """Contract on the return code.  True: judge the result."""
    OUTCOMES[impl][rc] += 1
    if rc == L.BP_OK:
        return True
    if rc == L.BP_EUNSUPPORTED and may_refuse:
        fails.check(torch.isnan(buf).all().item(), "%s: refused, but the destination was written" % what)
        return False
    fails.append("%s: return code %d (%s)" % (what, rc, L.load().bp_strerror(rc).decode()))
    return False


def _run_fp32(lib, host, cid, fails, kind):
    tr, ci, co, k, s, p, op, n, h, w = host.case
    ho, wo = S.out_shape(host.case)
    cv = L.Conv(*host.case[:7])
    st = G.stream()
    (y_ref, dx_ref, dw_ref, db_ref), (y_b, dx_b, dw_b, db_b) = host.f32()
    Ty, Tdx, Tdw, Tdb = host.T
    wd = G.dev(host.w)
    bd = G.dev(host.bias) if host.biased else None
    keep, pw = G.pointwise(*host.pw)
    packed = []
    for d in (L.PACK_FWD, L.PACK_BWD):
        nf = lib.bp_conv_packed_floats(C.byref(cv), d)
        if nf <= 0:
            fails.check(lib.bp_conv_kernel_id(C.byref(cv), d) == -1, "no packed image although a kernel id exists")
            packed.append(None)
            continue
        pk = torch.zeros(nf, device="cuda")
        rc = lib.bp_conv_pack(C.byref(cv), d, L.ptr(wd), L.ptr(pk), st)
        fails.check(rc == L.BP_OK, "bp_conv_pack(dir %d): %d" % (d, rc))
        packed.append(pk)
    xb, xv = _in_view(host.x, kind)
    dyb, dyv = _in_view(host.dy, kind)
    ws_bytes = lib.bp_conv_backward_weight_workspace(C.byref(cv), C.byref(xv), C.byref(dyv))
    fails.check(ws_bytes > 0, "no weight-gradient workspace")
    for name in ("direct", "mfma", "auto"):
        impl, refuse = IMPLS[name], name == "mfma"
        pf, pb = packed
        yb, yv = _out_view(n, co, ho, wo, kind)
        # (a direction without a matrix-core kernel has no packed image: BP_IMPL_MFMA has nothing to be called with)
        rc = L.BP_EUNSUPPORTED if refuse and pf is None else \
            lib.bp_conv_forward(C.byref(cv), C.byref(xv), C.byref(pw), L.ptr(pf), L.ptr(wd), L.ptr(bd), C.byref(yv), impl, st)
        if _outcome(fails, name, rc, "%s forward [%s]" % (name, kind), yb, yv, refuse):
            got, clean = _read(yb, yv)
            fails.check(clean, "%s forward [%s]: stores outside the view" % (name, kind))
            _judge(fails, cid, name, "y", got, y_ref, y_b, Ty, False, kind)
        dxb, dxv = _out_view(n, ci, h, w, kind)
        rc = L.BP_EUNSUPPORTED if refuse and pb is None else \
            lib.bp_conv_backward_data(C.byref(cv), C.byref(dyv), L.ptr(pb), L.ptr(wd), C.byref(dxv), impl, st)
        if _outcome(fails, name, rc, "%s backward_data [%s]" % (name, kind), dxb, dxv, refuse):
            got, clean = _read(dxb, dxv)
            fails.check(clean, "%s backward_data [%s]: stores outside the view" % (name, kind))
            _judge(fails, cid, name, "dx", got, dx_ref, dx_b, Tdx, False, kind)
        ws = torch.zeros(ws_bytes // 8 + 8, dtype=torch.float64, device="cuda")
        dw = torch.full(host.w.shape, float("nan"), device="cuda")
        db = torch.full((co,), float("nan"), device="cuda") if host.biased else None
        rc = lib.bp_conv_backward_weight(C.byref(cv), C.byref(xv), C.byref(pw), C.byref(dyv), L.ptr(dw), L.ptr(db),
                                         L.ptr(ws), ws.numel() * 8, impl, st)
        if _outcome(fails, name, rc, "%s backward_weight [%s]" % (name, kind), dw, None, refuse):
            _judge(fails, cid, name, "dw", dw.cpu().numpy().astype(np.float64), dw_ref, dw_b, Tdw, False, kind)
            if host.biased:
                _judge(fails, cid, name, "dbias", db.cpu().numpy().astype(np.float64), db_ref, db_b, Tdb, False, kind)
        elif host.biased:
            fails.check(torch.isnan(db).all().item(), "%s backward_weight [%s]: refused, but dbias was written" % (name, kind))


def _run_bf16(lib, host, cid, fails, kind, in_bf, out_bf):
    """BP_IMPL_BF16 with views of the given element types.  `kind` "odd" keeps no alignment the kernels ask for: what
    bp_conv_bf16_supported refuses for the actual views must be refused by the call."""
    tr, ci, co, k, s, p, op, n, h, w = host.case
    ho, wo = S.out_shape(host.case)
    cv = L.Conv(*host.case[:7])
    st = G.stream()
    (y_ref, dx_ref, dw_ref, _), (y_b, dx_b, dw_b, _) = host.bf16(in_bf)
    Ty, Tdx, Tdw, _ = host.T
    where = "%s %s-%s" % (kind, "bf16" if in_bf else "f32", "bf16" if out_bf else "f32")
    x_in, dy_in = host.bf16_operands(in_bf)
    wd = G.dev(host.w)
    bd = G.dev(host.bias) if host.biased else None
    keep, pw = G.pointwise(*host.pw)
    xb, xv = _in_view(x_in, kind, in_bf)
    dyb, dyv = _in_view(dy_in, kind, in_bf)
    packed = []
    for d in (L.PACK_FWD, L.PACK_BWD):
        ne = lib.bp_conv_bf16_packed_elems(C.byref(cv), d)
        if ne <= 0:
            packed.append(None)
            continue
        pk = torch.zeros(ne, device="cuda", dtype=torch.bfloat16)
        rc = lib.bp_conv_bf16_pack(C.byref(cv), d, L.ptr(wd), L.ptr(pk), st)
        fails.check(rc == L.BP_OK, "bp_conv_bf16_pack(dir %d): %d" % (d, rc))
        packed.append(pk)
    if packed[0] is not None:
        yb, yv = _out_view(n, co, ho, wo, kind, out_bf)
        sup = lib.bp_conv_bf16_supported(C.byref(cv), L.PACK_FWD, C.byref(xv), C.byref(yv))
        rc = lib.bp_conv_forward(C.byref(cv), C.byref(xv), C.byref(pw), L.ptr(packed[0]), L.ptr(wd), L.ptr(bd), C.byref(yv),
                                 L.IMPL_BF16, st)
        fails.check(sup == 1 or rc == L.BP_EUNSUPPORTED, "bf16 forward [%s]: views refused by bp_conv_bf16_supported ran (%d)" % (where, rc))
        fails.check(not (sup == 1 and not host.biased) or rc == L.BP_OK, "bf16 forward [%s]: supported, but returned %d" % (where, rc))
        if _outcome(fails, "bf16", rc, "bf16 forward [%s]" % where, yb, yv, True):
            got, clean = _read(yb, yv)
            fails.check(clean, "bf16 forward [%s]: stores outside the view" % where)
            _judge(fails, cid, "bf16", "y", got, y_ref, y_b, Ty, out_bf, where)
    if packed[1] is not None:
        dxb, dxv = _out_view(n, ci, h, w, kind, out_bf)
        sup = lib.bp_conv_bf16_supported(C.byref(cv), L.PACK_BWD, C.byref(dyv), C.byref(dxv))
        rc = lib.bp_conv_backward_data(C.byref(cv), C.byref(dyv), L.ptr(packed[1]), L.ptr(wd), C.byref(dxv), L.IMPL_BF16, st)
        # (the one-channel head kernel of conv_bf16_head.hip reads with scalar loads and takes views that the tiled
        #  kernels, which bp_conv_bf16_supported answers for, refuse: the library says where it applies)
        head = lib.bp_conv_backward_data_act_workspace(C.byref(cv), C.byref(dyv), C.byref(dxv)) > 0
        fails.check(sup == 1 or rc == L.BP_EUNSUPPORTED or head,
                    "bf16 backward_data [%s]: views refused by bp_conv_bf16_supported ran (%d)" % (where, rc))
        fails.check(sup != 1 or rc == L.BP_OK, "bf16 backward_data [%s]: supported, but returned %d" % (where, rc))
        if _outcome(fails, "bf16", rc, "bf16 backward_data [%s]" % where, dxb, dxv, True):
            got, clean = _read(dxb, dxv)
            fails.check(clean, "bf16 backward_data [%s]: stores outside the view" % where)
            _judge(fails, cid, "bf16", "dx", got, dx_ref, dx_b, Tdx, out_bf, where)
    if out_bf:
        return                                                # (the weight gradient has no produced view: once per input type)
    ws_bytes = lib.bp_conv_backward_weight_workspace(C.byref(cv), C.byref(xv), C.byref(dyv))
    ws = torch.zeros(ws_bytes // 8 + 8, dtype=torch.float64, device="cuda")
    dw = torch.full(host.w.shape, float("nan"), device="cuda")
    rc = lib.bp_conv_backward_weight(C.byref(cv), C.byref(xv), C.byref(pw), C.byref(dyv), L.ptr(dw), None, L.ptr(ws),
                                     ws.numel() * 8, L.IMPL_BF16, st)
    if _outcome(fails, "bf16", rc, "bf16 backward_weight [%s]" % where, dw, None, True):
        _judge(fails, cid, "bf16", "dw", dw.cpu().numpy().astype(np.float64), dw_ref, dw_b, Tdw, False, where)
    if host.biased:       # the bf16 path has no bias gradient: refused, nothing written
        db = torch.full((co,), float("nan"), device="cuda")
        dw2 = torch.full(host.w.shape, float("nan"), device="cuda")
        rc = lib.bp_conv_backward_weight(C.byref(cv), C.byref(xv), C.byref(pw), C.byref(dyv), L.ptr(dw2), L.ptr(db), L.ptr(ws),
                                         ws.numel() * 8, L.IMPL_BF16, st)
        fails.check(rc == L.BP_EUNSUPPORTED and torch.isnan(db).all().item() and torch.isnan(dw2).all().item(),
                    "bf16 backward_weight with dbias [%s]: %d" % (where, rc))


def _run_all(lib, host, cid, fails):
    cv = L.Conv(*host.case[:7])
    any_bf16 = any(lib.bp_conv_bf16_supported(C.byref(cv), d, None, None) == 1 for d in (L.PACK_FWD, L.PACK_BWD))
    for kind in ("aligned", "odd"):
        _run_fp32(lib, host, cid, fails, kind)
    if any_bf16:
        for in_bf, out_bf in ((True, True), (False, True), (True, False), (False, False)):
            _run_bf16(lib, host, cid, fails, "aligned", in_bf, out_bf)
        for in_bf, out_bf in ((True, True), (False, False)):
            _run_bf16(lib, host, cid, fails, "odd", in_bf, out_bf)
    torch.cuda.synchronize()


def _check_switch(lib, host, fails, setting):
    """The ws:* cases have the widths the weights-stationary kernels take: with the switch on, bp_conv_ws_kind (which
    follows bp_set_option) must name such a kernel for the views of this test, and none with it off -- otherwise both
    settings would silently run the tiled kernel."""
    tr, ci, co, k, s, p, op, n, h, w = host.case
    ho, wo = S.out_shape(host.case)
    cv = L.Conv(*host.case[:7])
    kinds = []
    for bf in ((False, True) if b"f32_ws" in SWITCHES[tuple(host.case[:7])] else (True,)):
        for d, (cg, hg, wg, cp, hp, wp) in ((L.PACK_FWD, (ci, h, w, co, ho, wo)), (L.PACK_BWD, (co, ho, wo, ci, h, w))):
            ib, iv = _out_view(n, cg, hg, wg, "aligned", bf)
            ob, ov = _out_view(n, cp, hp, wp, "aligned", bf)
            kinds.append(lib.bp_conv_ws_kind(C.byref(cv), d, C.byref(iv), C.byref(ov)))
    if setting == 1:
        fails.check(all(kd > 0 for kd in kinds), "switch on: bp_conv_ws_kind = %s, a case meant for the stationary kernels" % kinds)
    else:
        fails.check(all(kd == 0 for kd in kinds), "switch off: bp_conv_ws_kind = %s" % kinds)


@pytest.mark.parametrize("index", range(len(TAGGED)), ids=[S.case_id(t, c) for t, c in TAGGED])
def test_convolution_sweep(index):
    lib = L.load()
    host = Host(index)
    cid = S.case_id(*TAGGED[index])
    fails = Failures()
    switches = SWITCHES.get(tuple(host.case[:7]), ())
    try:
        for setting in ((1, 0) if switches else (None,)):
            for name in switches:
                assert lib.bp_set_option(name, setting) == 0
            before = len(fails)
            if host.tag.startswith("ws:"):
                _check_switch(lib, host, fails, setting)
            _run_all(lib, host, cid, fails)
            if switches:
                fails[before:] = ["[%s = %d] %s" % (b", ".join(switches).decode(), setting, f) for f in fails[before:]]
    finally:
        for name in switches:
            lib.bp_set_option(name, -1)
    RAN.add(index)
    assert not fails, "%s: %d failures\n  " % (cid, len(fails)) + "\n  ".join(fails[:40])


def test_sweep_report():
    """Outcomes per implementation and the worst ratio to each limit over the cases that ran in this process (-s).
    A report: under -k it covers the selected cases only.  When the whole file ran, every case must have been counted
    and BP_IMPL_DIRECT / BP_IMPL_AUTO must have served every call."""
    print()
    for impl in IMPLS:
        oc = OUTCOMES[impl]
        print("%-6s BP_OK %6d   BP_EUNSUPPORTED %6d   other %d" % (impl, oc[L.BP_OK], oc[L.BP_EUNSUPPORTED],
                                                                  sum(v for k, v in oc.items() if k not in (L.BP_OK, L.BP_EUNSUPPORTED))))
    for key in sorted(WORST):
        print("worst %-12s %-6s %-5s %8.3f of the limit   %s" % (key + WORST[key]))
    print("%d of %d cases ran in this process" % (len(RAN), len(TAGGED)))
    for impl in ("direct", "auto"):
        assert set(OUTCOMES[impl]) <= {L.BP_OK}, "BP_IMPL_%s must serve every case" % impl.upper()
    if len(RAN) == len(TAGGED):
        # per case and layout: forward, data gradient, weight gradient (twice each for the switched ws:* cases)
        calls = 6 * (len(TAGGED) + sum(1 for t, c in TAGGED if tuple(c[:7]) in SWITCHES))
        for impl in ("direct", "mfma", "auto"):
            assert sum(OUTCOMES[impl].values()) == calls, (impl, sum(OUTCOMES[impl].values()), calls)
        assert OUTCOMES["bf16"][L.BP_OK] > 0 and OUTCOMES["mfma"][L.BP_OK] > 0.9 * calls
