#!/usr/bin/env python3
"""Time bp_unary_forward (kind 1, tanh) and bp_unary_backward by HIP events on the three views a CVAE meets:

    dense16   (64, 512, 512, 16) dense            an interior 16-channel layer at full resolution
    head1     (64, 512, 512, 1) dense             a head's one-channel output
    slice16   (64, 512, 512, 16) at channel 16 of a 32-wide buffer

    python tools/unary_bench.py --parent /path/to/parent/libbp_hip.so [--lib other/libbp_hip.so] [--reps 20] [--n 64]
                                [--size 512]

The yardstick for the forward is the PARENT commit's bp_unary_forward (one scalar element per thread) from a library
built from that commit, on the same views in the same process: the two alternate in groups of launches, and the smaller
of each one's two group medians is reported.  ``--lib`` times another build of the library in place of the package's.

Bytes are the algorithm's: forward one read + one write, backward two reads + one write (one gradient contribution),
4 bytes each; the roof is the 6.29 TB/s float4 copy of the MI355X.  Prints one JSON line per (view, kernel).

Only a run with ``--parent`` is the acceptance run: it compares the outputs of the two forwards bit for bit, then exits
non-zero if the new forward is slower than the parent's on any view (beyond 2 % of measurement spread).  Without
``--parent`` the tool only reports rates and checks nothing."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baryon_painter_amd import _lib as L  # noqa: E402

HBM_ROOF = 6.29e12


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def view_of(buf, c, coff):
    n, h, w, cs = buf.shape
    return L.View(buf.data_ptr(), n, h, w, c, cs, coff, L.F32)


def timed(fn, reps):
    """Median time in seconds of ``fn()`` over ``reps`` event-timed launches (after two warm-up launches)."""
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libbp_hip.so built from the parent commit (its bp_unary_forward is the yardstick); "
                                     "only a run with it checks 'not slower than the parent' -- the acceptance run")
    ap.add_argument("--lib", help="the library under test (default: the one built in the package)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unary_bench needs a GPU")
    lib = L.load()
    if a.lib:
        lib = C.CDLL(os.path.abspath(a.lib))
        for name in ("bp_unary_forward", "bp_unary_backward"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = L.SIGNATURES[name]
    parent = None
    if a.parent:
        parent = C.CDLL(os.path.abspath(a.parent))
        parent.bp_unary_forward.restype, parent.bp_unary_forward.argtypes = L.SIGNATURES["bp_unary_forward"]
    n, s = a.n, a.size
    views = {"dense16": (16, 16, 0), "head1": (1, 1, 0), "slice16": (16, 32, 16)}
    slower = []
    for name, (c, cs, co) in views.items():
        x = torch.randn((n, s, s, cs), device="cuda")
        y = torch.zeros_like(x)
        y2 = torch.zeros_like(x)
        d = torch.randn((n, s, s, cs), device="cuda")
        g = torch.zeros_like(x)
        xv, yv, y2v, dv, gv = (view_of(t, c, co) for t in (x, y, y2, d, g))
        elems = n * s * s * c

        def fwd(lb, out):
            L.check(lb.bp_unary_forward(C.byref(xv), None, 1, C.byref(out), stream()), "unary_forward")

        def bwd():
            L.check(lib.bp_unary_backward(C.byref(dv), None, C.byref(yv), 1, C.byref(gv), stream()), "unary_backward")

        rows = {}
        if parent is not None:
            fwd(parent, y2v)
            fwd(lib, yv)
            torch.cuda.synchronize()
            assert torch.equal(y, y2), f"{name}: the new forward differs from the parent's"
            # alternate the two so that neither owns a quieter stretch of the machine
            half = max(a.reps // 2, 3)
            p1, n1 = timed(lambda: fwd(parent, y2v), half), timed(lambda: fwd(lib, yv), half)
            p2, n2 = timed(lambda: fwd(parent, y2v), half), timed(lambda: fwd(lib, yv), half)
            rows["forward_parent"] = (min(p1[0], p2[0]), 2)
            rows["forward"] = (min(n1[0], n2[0]), 2)
        else:
            fwd(lib, yv)
            rows["forward"] = (timed(lambda: fwd(lib, yv), a.reps)[0], 2)
        rows["backward"] = (timed(bwd, a.reps)[0], 3)
        for kernel, (t, passes) in rows.items():
            nbytes = passes * 4 * elems
            print(json.dumps({"view": name, "shape": [n, s, s, c], "cstride": cs, "coff": co, "kernel": kernel,
                              "ms": round(t * 1e3, 4), "GB/s": round(nbytes / t / 1e9, 1),
                              "hbm_roof_fraction": round(nbytes / t / HBM_ROOF, 3)}), flush=True)
        if parent is not None and rows["forward"][0] > 1.02 * rows["forward_parent"][0]:
            slower.append(name)
        del x, y, y2, d, g
        torch.cuda.empty_cache()
    if slower:
        sys.exit(f"the new forward is slower than the parent's on: {slower}")


if __name__ == "__main__":
    main()
