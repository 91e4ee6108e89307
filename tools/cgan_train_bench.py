"""CGAN training: ``train_dtype`` fp32 against bf16 at the fiducial geometry (tile 512, nine blocks), in ONE process.

    python tools/cgan_train_bench.py [--batches 6 64] [--repeats 9] [--iters 3] [--json PATH]

Per batch size, after two warm-up iterations of every variant, REPEATS rounds; a round times ITERS training iterations of
each variant in turn (host clock around work that ends in a device synchronise), so drifts of the machine fall on all
variants alike.  Variants: fp32; bf16 with the column-strip weight gradient (bp_set_option("BP_BF16_WGRAD_WS", 1)); bf16
with the tiled weight gradient (... 0).  Then, alone, with device events: the trunk layer's weight gradient at
(batch, 128, 128), strip kernel against tiled kernel, and bp_view_cast in its four uses.  Medians and ranges are printed,
and one JSON line at the end.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from baryon_painter_amd import _lib as L                            # noqa: E402
from baryon_painter_amd.models.cgan import CGAN                     # noqa: E402
from baryon_painter_amd.utils import synthetic as syn               # noqa: E402

TILE, N_RES = 512, 9
OPTION = b"BP_BF16_WGRAD_WS"


def stat(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def trainer(train_dtype, batch):
    torch.manual_seed(0)
    m = CGAN(tile_size=TILE, device="cuda:0", n_res=N_RES, train_dtype=train_dtype)
    m.train(True)
    x, y, z = syn.synthetic_batch(batch, TILE, TILE, seed=5)
    args = (torch.from_numpy(np.tanh(3 * x - 0.5).astype(np.float32)).cuda(), torch.from_numpy(y).cuda(),
            torch.from_numpy(z).cuda(), torch.optim.Adam(m.g_parameters(), lr=5e-5, betas=(0.5, 0.999)),
            torch.optim.Adam(m.d_parameters(), lr=5e-5, betas=(0.5, 0.999)))
    return lambda: m.train_step(*args)


def iterations(lib, batch, repeats, iters):
    """ms per iteration of the three variants, interleaved."""
    steps = {"fp32": trainer("fp32", batch), "bf16": trainer("bf16", batch)}
    variants = [("fp32", "fp32", -1), ("bf16_strips", "bf16", 1), ("bf16_tiled", "bf16", 0)]
    times = {v[0]: [] for v in variants}
    try:
        for r in range(repeats + 1):
            for name, key, opt in variants:
                lib.bp_set_option(OPTION, opt)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(2 if r == 0 else iters):
                    steps[key]()
                torch.cuda.synchronize()
                if r:                                   # (round 0: the warm-up of every variant)
                    times[name].append((time.perf_counter() - t0) * 1e3 / iters)
    finally:
        lib.bp_set_option(OPTION, -1)
    return {k: stat(v) for k, v in times.items()}


def events(fn, repeats, rep):
    out = []
    for r in range(repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rep):
            L.check(fn())
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            out.append(e0.elapsed_time(e1) * 1e3 / rep)
    return out


def wgrad_alone(lib, batch, repeats):
    """us per call (partial sums + reduction) of the trunk layer's weight gradient with a pending pointwise on X."""
    n, h, w, c = batch, TILE // 4, TILE // 4, 128
    cv = L.Conv(0, c, c, 3, 1, 1, 0)
    x = torch.randn((n, h, w, c), device="cuda").to(torch.bfloat16)
    dy = torch.randn((n, h, w, c), device="cuda").to(torch.bfloat16)
    xv = L.View(x.data_ptr(), n, h, w, c, c, 0, L.BF16)
    dyv = L.View(dy.data_ptr(), n, h, w, c, c, 0, L.BF16)
    pwk = [torch.rand(c, device="cuda") + 0.5, torch.rand(c, device="cuda") - 0.5, torch.full((c,), 0.2, device="cuda")]
    pw = L.Pointwise(*[t.data_ptr() for t in pwk])
    nb = lib.bp_conv_backward_weight_workspace(C.byref(cv), C.byref(xv), C.byref(dyv))
    ws = torch.zeros(nb // 4 + 64, device="cuda")
    dw = torch.zeros((c, c, 3, 3), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        return lib.bp_conv_backward_weight(C.byref(cv), C.byref(xv), C.byref(pw), C.byref(dyv), L.ptr(dw), None, L.ptr(ws), nb,
                                           L.IMPL_BF16, st)
    times, got = {"strips": [], "tiled": []}, {}
    try:
        for r in range(repeats):                        # alternating, one process
            for name, opt in (("strips", 1), ("tiled", 0)):
                lib.bp_set_option(OPTION, opt)
                times[name] += events(call, 1, 10)
                got[name] = dw.clone()
    finally:
        lib.bp_set_option(OPTION, -1)
    flop = 2.0 * n * h * w * 9 * c * c
    out = {k: dict(stat(v), tflops=flop / np.median(v) / 1e6) for k, v in times.items()}
    out["max_rel_difference"] = float((got["strips"] - got["tiled"]).abs().max() / got["tiled"].abs().max())
    return out


def cast_alone(lib, batch, repeats):
    """us per call of bp_view_cast on the trunk tensor: entry (fp32 + pointwise -> bf16), exit (bf16 -> fp32) and their
    backward passes (fp32 -> bf16, bf16 -> fp32), with the bytes each moves."""
    n, h, w, c = batch, TILE // 4, TILE // 4, 128
    f = torch.randn((n, h, w, c), device="cuda")
    b = torch.zeros((n, h, w, c), device="cuda", dtype=torch.bfloat16)
    fv = L.View(f.data_ptr(), n, h, w, c, c, 0, L.F32)
    bv = L.View(b.data_ptr(), n, h, w, c, c, 0, L.BF16)
    pwk = [torch.rand(c, device="cuda") + 0.5, torch.rand(c, device="cuda") - 0.5, torch.full((c,), 0.2, device="cuda")]
    pw = L.Pointwise(*[t.data_ptr() for t in pwk])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    legs = {"fp32+pointwise->bf16": lambda: lib.bp_view_cast(C.byref(fv), C.byref(pw), C.byref(bv), st),
            "fp32->bf16": lambda: lib.bp_view_cast(C.byref(fv), None, C.byref(bv), st),
            "bf16->fp32": lambda: lib.bp_view_cast(C.byref(bv), None, C.byref(fv), st)}
    nbytes = 6.0 * n * h * w * c
    out = {}
    for k, fn in legs.items():
        t = events(fn, repeats, 20)
        out[k] = dict(stat(t), gb_per_s=nbytes / np.median(t) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[6, 64])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("at least seven repeats")
    if not torch.cuda.is_available():
        raise SystemExit("cgan_train_bench needs a GPU")
    lib = L.load()
    result = {"tile": TILE, "n_res": N_RES, "repeats": a.repeats, "iters": a.iters, "device": torch.cuda.get_device_name(0),
              "batches": {}}
    for batch in a.batches:
        it = iterations(lib, batch, a.repeats, a.iters)
        gc.collect()                    # (a model and its plans reference each other)
        torch.cuda.empty_cache()
        row = {"iteration_ms": it, "tiles_per_s": {k: batch / v["median"] * 1e3 for k, v in it.items()},
               "wgrad_us": wgrad_alone(lib, batch, a.repeats), "view_cast_us": cast_alone(lib, batch, a.repeats)}
        result["batches"][str(batch)] = row
        print(f"batch {batch}: tile {TILE}, {N_RES} blocks; median [min, max] over {a.repeats} rounds of {a.iters} iterations")
        for k, v in it.items():
            print(f"  {k:12s} {v['median']:8.2f} ms [{v['min']:.2f}, {v['max']:.2f}]  {row['tiles_per_s'][k]:8.1f} tiles/s")
        wg = row["wgrad_us"]
        for k in ("strips", "tiled"):
            print(f"  trunk weight gradient ({batch}, 128, 128) {k:7s} {wg[k]['median']:8.1f} us [{wg[k]['min']:.1f}, "
                  f"{wg[k]['max']:.1f}]  {wg[k]['tflops']:6.1f} TF/s")
        print(f"    largest difference between the two / largest element: {wg['max_rel_difference']:.2e}")
        for k, v in row["view_cast_us"].items():
            print(f"  bp_view_cast {k:22s} {v['median']:8.1f} us [{v['min']:.1f}, {v['max']:.1f}]  {v['gb_per_s']:7.0f} GB/s",
                  flush=True)
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
