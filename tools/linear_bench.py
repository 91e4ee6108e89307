#!/usr/bin/env python3
"""Time the fully connected layer's kernels (csrc/linear.hip) and what a dense bottleneck costs a model.

    python tools/linear_bench.py [--kernels-only] [--steps 20] [--warmup 5] [--paint-tiles 2048] [--runs 1]

1. The three kernels alone at the 512^2 bottleneck, K = 16 384, O in {32, 512}, n in {4, 64, 256}: HIP events after
   warm-up, median of 20 launches, beside their traffic floor -- one pass over the 4*O*K bytes of the weight matrix
   (read by the forward and the data gradient, written by the weight gradient) at the nominal 8 TB/s of HBM3E.
2. The training step (batch 64 of 512^2 tiles, fp32 and bf16) of the fiducial architecture and of its dense-tail twin --
   q_x_y_out / prior_z_y end in ``flatten, linear -> 512, unflatten (2, 1, 16, 16)`` instead of the k5 convolution --
   in the same process, timed as bench.py times its train leg (eager steps, FlatAdam).
3. ``paint_stream`` of both, as bench.py's paint leg runs it (raw host tiles in, physical host tiles out).
One JSON line per figure on stdout.  ``--runs R`` repeats each model figure R times in this process and prints all.
"""
import argparse
import contextlib
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baryon_painter_amd import _lib as L                                    # noqa: E402
from baryon_painter_amd.models import arch as A                             # noqa: E402
from baryon_painter_amd.utils import synthetic as syn                       # noqa: E402

HBM_NOMINAL = 8.0e12        # bytes / s


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def median_ms(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernels():
    lib = L.load()
    c, h, w = 64, 16, 16
    K = c * h * w
    for O in (32, 512):
        for n in (4, 64, 256):
            d = L.Linear(K, O, c, h, w, O, 1, 1, 1)
            x = torch.randn((n, h, w, c), device="cuda")
            y = torch.zeros((n, 1, 1, O), device="cuda")
            dy = torch.randn((n, 1, 1, O), device="cuda")
            dx = torch.zeros_like(x)
            wt = torch.randn((O, K), device="cuda") / K ** 0.5
            b = torch.zeros(O, device="cuda")
            dw, db = torch.zeros_like(wt), torch.zeros_like(b)
            xv, yv = L.View(x.data_ptr(), n, h, w, c, c, 0), L.View(y.data_ptr(), n, 1, 1, O, O, 0)
            dyv, dxv = L.View(dy.data_ptr(), n, 1, 1, O, O, 0), L.View(dx.data_ptr(), n, h, w, c, c, 0)
            nb = int(lib.bp_linear_workspace(n, C.byref(d)))
            ws = torch.zeros(nb // 4 + 4, device="cuda")
            calls = {
                "forward": lambda: L.check(lib.bp_linear_forward(C.byref(d), C.byref(xv), None, L.ptr(wt), L.ptr(b),
                                                                 C.byref(yv), L.ptr(ws), nb, stream()), "forward"),
                "backward_data": lambda: L.check(lib.bp_linear_backward_data(C.byref(d), C.byref(dyv), L.ptr(wt),
                                                                             C.byref(dxv), stream()), "backward_data"),
                "backward_weight": lambda: L.check(lib.bp_linear_backward_weight(C.byref(d), C.byref(xv), None,
                                                                                 C.byref(dyv), L.ptr(dw), L.ptr(db),
                                                                                 stream()), "backward_weight"),
            }
            floor_us = 4 * O * K / HBM_NOMINAL * 1e6
            for name, fn in calls.items():
                med, lo, hi = median_ms(fn)
                print(json.dumps({"kernel": name, "K": K, "O": O, "n": n, "median_us": round(med * 1e3, 2),
                                  "min_us": round(lo * 1e3, 2), "max_us": round(hi * 1e3, 2),
                                  "floor_us": round(floor_us, 2), "fraction_of_floor": round(floor_us / (med * 1e3), 3),
                                  "workspace_bytes": nb if name == "forward" else 0}), flush=True)


def dense_twin(tile):
    """The fiducial architecture with the k5 convolution at the end of q_x_y_out / prior_z_y replaced by
    flatten, linear -> 2 * prod(dim_z), unflatten (2, *dim_z)."""
    a = A.fiducial_architecture(tile)
    zs = tile // 32
    out = 2 * zs * zs
    a["q_x_y_out"] = [("flatten",), ("linear", {"in_features": 64 * zs * zs, "out_features": out}),
                      ("unflatten", (2, 1, zs, zs))]
    stem = A.conv_down(in_channel=2, channels=[8, 16, 32], scales=[2, 4, 4])
    a["prior_z_y"] = stem + [("flatten",), ("linear", {"in_features": 32 * zs * zs, "out_features": out}),
                             ("unflatten", (2, 1, zs, zs))]
    return a


def train_ms(arch, dtype, tile, n, steps, warmup):
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.optim import FlatAdam
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(sys.stderr):
        model = CVAE(arch, "cuda:0", dtype=dtype)
    opt = FlatAdam(model, lr=1e-3)
    nb = min(n, 8)
    x, y, aux = syn.synthetic_batch(nb, tile, tile, seed=1234)
    reps = (n + nb - 1) // nb
    x = torch.from_numpy(np.tile(x, (reps, 1, 1, 1))[:n]).cuda()
    y = torch.from_numpy(np.tile(y, (reps, 1, 1, 1))[:n]).cuda()
    aux = torch.from_numpy(np.tile(aux, reps)[:n]).cuda()

    def step():
        elbo = model(x, y, aux)
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
        return elbo
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        elbo = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert np.isfinite(float(elbo.detach()))
    return model, ms


def paint_rate(model, dtype, tile, n_paint):
    from baryon_painter_amd.painter import CVAEPainter
    from baryon_painter_amd.utils.datasets import SyntheticTileDataset
    model.train(False)
    pb = 256 if dtype == "bf16" else 128
    ds = SyntheticTileDataset(n_sample=8, tile_size=tile, seed=3)
    pt = CVAEPainter.__new__(CVAEPainter)
    pt.model, pt.compute_device, pt.sync = model, torch.device("cuda:0"), None
    pt.input_field, pt.label_fields = ds.input_field, ds.label_fields
    pt.transform, pt.inverse_transform = ds.transform, ds.inverse_transform
    raw = np.stack([ds.raw_fields(i)[0] for i in range(8)])
    zs = np.array([ds.raw_fields(i)[2] for i in range(8)])
    reps = (n_paint + 7) // 8
    tin = torch.from_numpy(np.tile(raw, (reps, 1, 1))[:n_paint]).pin_memory()
    zin = np.tile(zs, reps)[:n_paint]
    tout = torch.empty((n_paint, tile, tile), dtype=torch.float32).pin_memory()
    ids = np.arange(n_paint, dtype=np.int64)
    with torch.no_grad():
        pt.paint_stream(tin[:2 * pb], zin[:2 * pb], batch_size=pb, tile_ids=ids[:2 * pb], out=tout[:2 * pb])   # capture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pt.paint_stream(tin, zin, batch_size=pb, tile_ids=ids, out=tout)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert np.isfinite(tout.numpy()).all()
    return n_paint / dt


def models(args):
    tile, n = args.tile, args.batch
    for dtype in ("f32", "bf16"):
        for name, arch in (("fiducial", A.fiducial_architecture(tile)), ("dense-tail twin", dense_twin(tile))):
            for run in range(args.runs):
                model, ms = train_ms(arch, dtype, tile, n, args.steps, args.warmup)
                print(json.dumps({"model": name, "dtype": dtype, "run": run, "train_ms_per_step": round(ms, 3),
                                  "train_tiles_per_s": round(n / ms * 1e3, 1), "batch": n, "tile": tile,
                                  "parameters": model.count_parameters()}), flush=True)
                if args.paint_tiles > 0:
                    rate = paint_rate(model, dtype, tile, args.paint_tiles)
                    print(json.dumps({"model": name, "dtype": dtype, "run": run, "paint_tiles_per_s": round(rate, 1),
                                      "paint_tiles": args.paint_tiles}), flush=True)
                del model
                gc.collect()
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--paint-tiles", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=1)
    args = ap.parse_args()
    kernels()
    if not args.kernels_only:
        models(args)


if __name__ == "__main__":
    main()
