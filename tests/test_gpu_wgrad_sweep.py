"""GPU: every weight-gradient kernel behind the C ABI where a split walks several tiles (tests/wgrad_sweep.py).

tests/test_gpu_conv_sweep.py draws tensors of at most 3 x 22 x 40: every workgroup of every weight-gradient kernel has
exactly one tile there, and the second iteration of every tile loop -- the prefetch of tile + nsplit, the last
iteration without one, splits one tile short of their neighbours, consecutive tiles in different images, the 16-group
reduction, the second chunk of the self-reducing kernels' fold -- never runs.  The cases here reach those by extent
alone, in the production configuration (no environment switch, no subprocess), at every kernel instantiation the
dispatcher can pick; test_wgrad_sweep_host.py pins which kernel serves each and with how many splits.

Per case, BP_IMPL_MFMA, BP_IMPL_AUTO and BP_IMPL_MFMA | BP_IMPL_SHARED on a 16-byte addressable channel slice of a wider
buffer and on a slice with odd stride and offset, and BP_IMPL_BF16 wherever bp_conv_backward_weight_plan names a bf16
kernel for bf16 operands, fp32 operands and the case's own mix.  Each call:
  a. dW (and dbias on every third case) equals the float64 reference of the integer data EXACTLY; one call per case
     uses random normal data instead and is judged by conv_sweep_gpu._judge under the suite's limits;
  b. gets a workspace of exactly bp_conv_backward_weight_workspace bytes filled with NaN and followed by 256 bytes of
     NaN that must survive, and a dW filled with NaN that must come out free of it; with a workspace 4 bytes short
     (BP_IMPL_BF16, which asks for its own kernel's partial images only: 4 bytes short of those) the call returns
     BP_EWORKSPACE and leaves dW and dbias untouched;
  c. run twice gives the same bits.
One more test defers the reductions of every fp32 case of regimes A, C and R between one bp_wgrad_defer_begin and one
flush.  The report prints what ran and, when the whole file ran, requires every (family, regime) of the module served.

No case failed on its first run on the GPU: no kernel had to be fixed, and wgrad_sweep.REGRESSIONS is empty.  That the
sweep notices was checked once with the tap-packed kernel's prefetch condition made wrong on purpose (tile + 2 nsplit
in place of tile + nsplit, so a split's second tile is the first one again): regimes A and B of its cases failed with
every element of dW off by up to 5137, regime C -- one tile per split, all the older sweep reaches -- passed.

Wall time on one MI355X, both measured in one visit: this file 7 s (213 cases, the deferral test and the report),
tests/test_gpu_conv_sweep.py 63 s: no regime was thinned.  (The float64 reference runs on the device, as one batched
product per tap over chunks of 2048 pixels; as a single product per tap it took 375 s.)
"""
import collections
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import conv_sweep as S
import gpu_util as G
import wgrad_sweep as W
from conv_sweep_gpu import Failures, _judge
from golden import make_wgrad_plan as M

pytestmark = pytest.mark.gpu

# seconds of `pytest -m gpu` for this file / for tests/test_gpu_conv_sweep.py, measured in the same visit on one MI355X
WALL_TIME = {"test_gpu_wgrad_sweep.py": 7, "test_gpu_conv_sweep.py": 63}

GUARD = 256
SERVED = collections.Counter()         # (family, regime) -> calls that the listed kernel served in the listed regime
RAN = set()
SHARED_DIFFERS = set()                 # tags of tap-blocked cases whose plan under BP_IMPL_SHARED has another nsplit


def _view(t, kind, bf16=False):
    """An NHWC tensor as a channel slice of a wider buffer (poisoned outside the slice)."""
    n, h, w, c = t.shape
    cs, co = W.layout(c, kind, bf16)
    buf = torch.full((n, h, w, cs), 7.5, dtype=torch.float32, device="cuda")
    buf[..., co:co + c] = t
    if bf16:
        buf = buf.to(torch.bfloat16)
    return buf, L.View(buf.data_ptr(), n, h, w, c, cs, co, L.BF16 if bf16 else L.F32)


class Operands:
    """The views of one pair of tensors, made on demand: (kind, element types of (x, dy)) -> (x view, dy view)."""

    def __init__(self, x, dy):
        self.x, self.dy, self._v = x, dy, {}

    def views(self, kind, dt):
        out = []
        for t, name, b in ((self.x, "x", dt[0] == "b"), (self.dy, "dy", dt[1] == "b")):
            key = (name, kind, b)
            if key not in self._v:
                self._v[key] = _view(t, kind, b)
            out.append(self._v[key][1])
        return out


def _plan(lib, cv, xv, dyv, flag):
    out = (C.c_int32 * 4)()
    rc = lib.bp_conv_backward_weight_plan(C.byref(cv), C.byref(xv), C.byref(dyv), flag, out)
    return rc, (L.WGRAD_FAMILIES[out[0]] if out[0] >= 0 else None), out[1], out[2], out[3]


def _call(lib, case, cv, xv, pw, dyv, flag, dbias, short=0):
    """One bp_conv_backward_weight on NaN-filled dW, dbias and workspace: (rc, dW, dbias, guard intact)."""
    co = case[2]
    nb = lib.bp_conv_backward_weight_workspace(C.byref(cv), C.byref(xv), C.byref(dyv))
    assert nb > 0 and nb % 4 == 0
    ws = torch.full(((nb + GUARD) // 4,), float("nan"), device="cuda")
    dw = torch.full(S.weight_shape(case), float("nan"), device="cuda")
    db = torch.full((co,), float("nan"), device="cuda") if dbias else None
    rc = lib.bp_conv_backward_weight(C.byref(cv), C.byref(xv), C.byref(pw) if pw is not None else None, C.byref(dyv),
                                     L.ptr(dw), L.ptr(db), L.ptr(ws), nb - short, flag, G.stream())
    return rc, dw, db, bool(torch.isnan(ws[nb // 4:]).all())


def _runs(lib, e, cv):
    """[(impl, kind, dt, listed)]: what the case is run with; `listed`: the run the case's regime is claimed for."""
    out = [(impl, kind, "ff", e.impl == "mfma" and kind == e.kind and impl != "shared")
           for kind in ("aligned", "odd") for impl in ("mfma", "auto", "shared")]
    for kind in ("aligned", "odd"):
        for dt in dict.fromkeys(("bb", "ff") + ((e.dt,) if e.impl == "bf16" and kind == "aligned" else ())):
            xv, dyv = M.views(L, e.case, kind, dt)
            if _plan(lib, cv, xv, dyv, L.IMPL_BF16)[0] == L.BP_OK:
                out.append(("bf16", kind, dt, e.impl == "bf16" and kind == e.kind and dt == e.dt))
    return out


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


def _exact(what, got, ref):
    got = got.double()
    if not torch.equal(got, ref):
        bad = got != ref
        worst = (got - ref)[bad].abs().max().item() if not torch.isnan(got).any() else float("nan")
        pytest.fail("%s: %d of %d elements differ from the float64 reference of the integer data (largest difference %s)"
                    % (what, int(bad.sum()), ref.numel(), worst))


@pytest.mark.parametrize("index", range(len(W.ENTRIES)), ids=[W.case_id(e) for e in W.ENTRIES])
@_stop_on_fault
def test_weight_gradient_sweep(index):
    lib = L.load()
    e = W.ENTRIES[index]
    cid = W.case_id(e)
    cv = L.Conv(*e.case[:7])
    k = e.case[3]
    x, dy, pw_host = W.int_inputs(e.case, index, "cuda")
    assert W.magnitude_bound(dy, pw_host) < W.EXACT_LIMIT
    keep, pw = G.pointwise(*(v.numpy() for v in pw_host))
    ref = W.reference_dw(e.case, W.activated(x, pw_host), dy.double())
    db_ref = dy.double().sum(dim=(0, 1, 2))
    ops = Operands(x, dy)
    with_dbias = index % 3 == 0
    listed = None
    for impl, kind, dt, is_listed in _runs(lib, e, cv):
        flag = M.impl_flag(L, impl)
        what = "%s %s [%s %s]" % (cid, impl, kind, dt)
        xv, dyv = ops.views(kind, dt)
        rc, family, ns, cxp, cyp = _plan(lib, cv, xv, dyv, flag)
        assert rc == L.BP_OK, "%s: plan returned %d" % (what, rc)
        if impl == "bf16":
            assert family in W.BF16_FAMILIES, what
            if is_listed:
                assert (family, ns) == (W.INST[e.inst].family, W.nsplit(e.inst, e.case)), what
        elif e.impl == "mfma":
            inst = W.expected_inst(e, kind)                 # (the odd slice: the plain twin or the fall-back kernel)
            assert (family, ns) == (W.INST[inst].family, W.nsplit(inst, e.case, impl == "shared")), what
            if impl == "shared" and family in ("tiles", "tiles_dma") and ns != W.nsplit(inst, e.case):
                SHARED_DIFFERS.add(e.tag)
        dbias = with_dbias and impl != "bf16"
        # b. the workspace contract, a. exactness, c. determinism
        rc, dw, db, guard = _call(lib, e.case, cv, xv, pw, dyv, flag, dbias)
        assert rc == L.BP_OK, "%s: returned %d (%s)" % (what, rc, lib.bp_strerror(rc).decode())
        assert guard, "%s: stores behind the workspace" % what
        assert not torch.isnan(dw).any(), "%s: %d elements of dW are NaN" % (what, int(torch.isnan(dw).sum()))
        _exact(what + " dW", dw, ref)
        if dbias:
            _exact(what + " dbias", db, db_ref)
        rc, dw2, db2, guard = _call(lib, e.case, cv, xv, pw, dyv, flag, dbias)
        assert rc == L.BP_OK and guard and torch.equal(dw, dw2), "%s: the second call gave other bits" % what
        # (BP_IMPL_BF16 asks for its own kernel's partial images only, the first bytes of the query: 4 bytes short of those)
        nb = lib.bp_conv_backward_weight_workspace(C.byref(cv), C.byref(xv), C.byref(dyv))
        short = 4 if impl != "bf16" else nb - ns * k * k * cxp * cyp * 4 + 4
        rc, dw3, db3, guard = _call(lib, e.case, cv, xv, pw, dyv, flag, dbias, short=short)
        assert rc == L.BP_EWORKSPACE, "%s: returned %d with a workspace 4 bytes short" % (what, rc)
        assert torch.isnan(dw3).all() and (db3 is None or torch.isnan(db3).all()) and guard, "%s: refused, but wrote" % what
        if is_listed:
            listed = (impl, kind, dt, family)
            SERVED[(family, e.regime)] += 1
    assert listed is not None, "%s: the run the case is listed for did not happen" % cid
    # a. one call on random normal data, under the suite's limits (bf16: against the bf16-rounded operands)
    impl, kind, dt, family = listed
    gen = torch.Generator(device="cuda").manual_seed(1000 + index)
    xr = torch.randn(x.shape, generator=gen, device="cuda")
    dyr = torch.randn(dy.shape, generator=gen, device="cuda")
    ci = e.case[1]
    rng = np.random.Generator(np.random.PCG64([43, index]))
    scale, shift, slope = (rng.uniform(lo, hi, ci).astype(np.float32) for lo, hi in ((0.5, 1.5), (0.2, 0.6), (0.05, 0.3)))
    slope[2::3] = 0.0
    keep_r, pwr = G.pointwise(scale, shift, slope)
    pwr_host = tuple(torch.from_numpy(v) for v in (scale, shift, slope))
    b16 = impl == "bf16"
    if b16:                                  # (bf16 views hold rounded tensors; the kernel rounds what it stages)
        xr = xr.to(torch.bfloat16).float() if dt[0] == "b" else xr
        dyr = dyr.to(torch.bfloat16).float() if dt[1] == "b" else dyr
    xa = W.activated(xr, pwr_host, b16)
    dya = dyr.to(torch.bfloat16).double() if b16 else dyr.double()
    ref_r = W.reference_dw(e.case, xa, dya).cpu().numpy()
    bnd_r = W.reference_dw(e.case, xa.abs(), dya.abs()).cpu().numpy()
    T = W.terms_dw(e.case, "cuda").cpu().numpy()
    ops_r = Operands(xr, dyr)                 # (kept: the views hold addresses only)
    xv, dyv = ops_r.views(kind, dt)
    rc, dw, db, guard = _call(lib, e.case, cv, xv, pwr, dyv, M.impl_flag(L, impl), False)
    assert rc == L.BP_OK and guard
    fails = Failures()
    _judge(fails, cid, impl, "dw", dw.cpu().numpy().astype(np.float64), ref_r, bnd_r, T, False, "%s %s" % (kind, dt))
    assert not fails, "%s: %s" % (cid, "; ".join(fails))
    RAN.add(index)


@_stop_on_fault
def test_deferred_reductions_of_every_capped_fp32_case():
    """Every BP_IMPL_MFMA case of regimes A, C and R between one bp_wgrad_defer_begin and one flush, each with its own
    workspace: more than the 40 jobs of one batch launch, in both classes of the reduction.  For the kernels whose
    reduction can wait, dW is untouched until the flush; afterwards every dW has the bits of its undeferred call."""
    lib = L.load()
    st = G.stream()
    picked = [(i, e) for i, e in enumerate(W.ENTRIES) if e.impl == "mfma" and e.regime[0] in "ACR"]
    jobs = []
    for i, e in picked:
        cv = L.Conv(*e.case[:7])
        x, dy, pw_host = W.int_inputs(e.case, i, "cuda")
        keep, pw = G.pointwise(*(v.numpy() for v in pw_host))
        xb, xv = _view(x, e.kind)
        dyb, dyv = _view(dy, e.kind)
        rc, family, ns = _plan(lib, cv, xv, dyv, L.IMPL_MFMA)[:3]
        rc, want, _, guard = _call(lib, e.case, cv, xv, pw, dyv, L.IMPL_MFMA, False)
        assert rc == L.BP_OK and guard, W.case_id(e)
        nb = lib.bp_conv_backward_weight_workspace(C.byref(cv), C.byref(xv), C.byref(dyv))
        ws = torch.full(((nb + GUARD) // 4,), float("nan"), device="cuda")
        dw = torch.full(S.weight_shape(e.case), float("nan"), device="cuda")
        jobs.append((e, cv, (xb, dyb, keep), xv, dyv, pw, nb, ws, dw, want, family, ns))
    deferring = [j for j in jobs if j[10] in W.DEFERRING]
    assert len(deferring) > 40 and any(j[11] <= 64 for j in deferring) and any(j[11] > 64 for j in deferring)
    torch.cuda.synchronize()
    assert lib.bp_wgrad_defer_begin() == 0
    try:
        for e, cv, keep, xv, dyv, pw, nb, ws, dw, want, family, ns in jobs:
            rc = lib.bp_conv_backward_weight(C.byref(cv), C.byref(xv), C.byref(pw), C.byref(dyv), L.ptr(dw), None, L.ptr(ws), nb,
                                             L.IMPL_MFMA | L.IMPL_DEFER, st)
            assert rc == L.BP_OK, W.case_id(e)
        torch.cuda.synchronize()
        for j in deferring:
            assert torch.isnan(j[8]).all(), "%s: reduced before the flush" % W.case_id(j[0])
        assert lib.bp_wgrad_defer_flush(1, st) == 0
    except BaseException:
        lib.bp_wgrad_defer_flush(-1, None)
        raise
    torch.cuda.synchronize()
    for e, cv, keep, xv, dyv, pw, nb, ws, dw, want, family, ns in jobs:
        assert torch.equal(dw, want), "%s (%s, %d splits): deferred dW differs" % (W.case_id(e), family, ns)
        assert torch.isnan(ws[nb // 4:]).all(), W.case_id(e)


def test_wgrad_sweep_report():
    """What ran in this process (-s), per family and regime.  A report: under -k it covers the selected cases only.  When
    the whole file ran, every (family, regime) pair of the module was served by the family it names, and the plan under
    BP_IMPL_SHARED differed from the plain one for at least one tap-blocked case."""
    print()
    fams = sorted({f for f, _ in W.pairs()})
    regimes = sorted({r for _, r in W.pairs()})
    print("%-14s" % "family" + "".join("%6s" % r for r in regimes))
    for f in fams:
        print("%-14s" % f + "".join("%6s" % (SERVED[(f, r)] or ("-" if (f, r) not in W.pairs() else 0)) for r in regimes))
    print("%d of %d cases ran in this process; regime B left out: %s" % (len(RAN), len(W.ENTRIES), sorted(i for i, _ in W.DROPPED_B)))
    print("plan under BP_IMPL_SHARED differs for %d tap-blocked cases" % len(SHARED_DIFFERS))
    if len(RAN) == len(W.ENTRIES):
        unserved = [p for p in W.pairs() if not SERVED[p]]
        assert not unserved, unserved
        assert SHARED_DIFFERS
