"""bp_conv_backward_weight_plan over the cases of tests/wgrad_sweep.py.

    python tests/golden/make_wgrad_plan.py          # rewrites tests/golden/wgrad_plan.json

The query is host arithmetic (view pointers are looked at for their alignment only), so the rows are the same with and
without a GPU.  tests/test_wgrad_sweep_host.py recomputes them and requires equality entry by entry: a retuned cap, tile
or gate of a weight-gradient kernel shows there first, and the case it moved is re-picked in wgrad_sweep.LAYERS.

Per case, one row per entry of QUERIES -- (impl, kind of view, element types of (x, dy)) -- holding
[return code, family, nsplit, cxp, cyp, bp_conv_backward_weight_workspace].
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PATH = os.path.join(HERE, "wgrad_plan.json")

QUERIES = tuple(("%s:%s:ff" % (impl, kind), impl, kind, "ff") for kind in ("aligned", "odd") for impl in ("mfma", "shared", "auto")) + \
    tuple(("bf16:%s:%s" % (kind, dt), "bf16", kind, dt) for kind in ("aligned", "odd") for dt in ("bb", "ff", "bf", "fb"))


def impl_flag(L, impl):
    return {"mfma": L.IMPL_MFMA, "shared": L.IMPL_MFMA | L.IMPL_SHARED, "auto": L.IMPL_AUTO, "bf16": L.IMPL_BF16}[impl]


def views(L, case, kind, dt, px=0x10000, py=0x20000):
    """(module input view, dy view) of a case at the layouts of wgrad_sweep.layout()."""
    import conv_sweep as S
    import wgrad_sweep as W
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    xb, yb = dt[0] == "b", dt[1] == "b"
    xcs, xco = W.layout(ci, kind, xb)
    ycs, yco = W.layout(co, kind, yb)
    return (L.View(px, n, h, w, ci, xcs, xco, L.BF16 if xb else L.F32),
            L.View(py, n, ho, wo, co, ycs, yco, L.BF16 if yb else L.F32))


def plan(lib, L, case, impl, kind, dt, px=0x10000, py=0x20000):
    """[rc, family, nsplit, cxp, cyp, workspace bytes]"""
    cv = L.Conv(*case[:7])
    x, y = views(L, case, kind, dt, px, py)
    out = (C.c_int32 * 4)()
    rc = lib.bp_conv_backward_weight_plan(C.byref(cv), C.byref(x), C.byref(y), impl_flag(L, impl), out)
    return [rc] + list(out) + [lib.bp_conv_backward_weight_workspace(C.byref(cv), C.byref(x), C.byref(y))]


def compute():
    from baryon_painter_amd import _lib as L
    import wgrad_sweep as W
    lib = L.load()
    return [[plan(lib, L, e.case, impl, kind, dt) for _, impl, kind, dt in QUERIES] for e in W.ENTRIES]


def load():
    with open(PATH) as f:
        return json.load(f)


def main():
    import wgrad_sweep as W
    rows = compute()
    with open(PATH, "w") as f:
        f.write("{\n")
        f.write('"queries": %s,\n' % json.dumps([q[0] for q in QUERIES]))
        f.write('"tags": %s,\n' % json.dumps([e.tag for e in W.ENTRIES]))
        f.write('"cases": %s,\n' % json.dumps([list(e.case) for e in W.ENTRIES], separators=(",", ":")))
        f.write('"rows": [\n%s\n]\n}\n' % ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
    print("%d cases x %d queries -> %s (%d bytes)" % (len(rows), len(QUERIES), PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
