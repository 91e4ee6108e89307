"""What the problematic-tile report costs: lightcone.paint_plane(on_device=True, regularise_std=...) with
``return_problematic_tiles=True`` against the same call without it, alternating in one run, and the two kernels behind
the report (bp_tile_outliers, bp_tile_keep) alone on one batch.  Fiducial 512^2 architecture with synthetic weights (as
bench.py builds it), fp32: a 4096^2 plane of 225 tiles of 512^2 in batches of 64, delta resident on the device and
``out=`` a device tensor, so that only the report crosses the host link.  One JSON line.

``--baseline-only`` times the call without the report alone: it needs nothing this tool's commit added and so runs on
an older checkout too, which gives the figure for "the default path did not get slower".

Times are host clocks around work that ends in a device synchronise; kernel times are device events around ``--kreps``
launches.  Every figure is the median of ``--reps`` repeats with the smallest and the largest beside it.

Usage: python tools/outlier_bench.py [--reps 7] [--kreps 20] [--batch 64] [--std 3.0] [--cap 16] [--baseline-only]"""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from baryon_painter_amd import lightcone as LC  # noqa: E402

TILE, N_PLANE = 512, 4096


def make_painter(dev):
    from baryon_painter_amd.models import arch as A
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.painter import CVAEPainter
    from baryon_painter_amd.utils.datasets import SyntheticTileDataset
    arch = A.fiducial_architecture(TILE)
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(sys.stderr):
        model = CVAE(arch, dev, dtype="f32")
    model.train(False)
    ds = SyntheticTileDataset(n_sample=8, tile_size=TILE, seed=3)
    pt = CVAEPainter.__new__(CVAEPainter)
    pt.model, pt.compute_device, pt.sync, pt.dtype = model, dev, None, "f32"
    pt.input_field, pt.label_fields = ds.input_field, ds.label_fields
    pt.transform, pt.inverse_transform = ds.transform, ds.inverse_transform
    return pt


def spread(times):
    """Median, smallest and largest, in milliseconds."""
    t = np.sort(np.asarray(times)) * 1e3
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t[0]), 3), "max_ms": round(float(t[-1]), 3)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def kernel_times(batch, std, cap, reps, kreps):
    """Device time per launch of the two entry points on one batch of ``batch`` 512^2 tiles with one spike in every
    eighth tile (so that the keep copies ``min(cap, batch / 8)`` tiles)."""
    from baryon_painter_amd import _lib as L
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(5)
    painted = torch.randn((batch, TILE, TILE), device="cuda", generator=g)
    painted[::8, 7, 9] = 1e3
    raw = torch.randn((batch, TILE, TILE), device="cuda", generator=g)
    stats = torch.empty(2 * batch, dtype=torch.float64, device="cuda")
    counts = torch.empty(batch, dtype=torch.int32, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
    index = torch.empty(cap, dtype=torch.int32, device="cuda")
    kraw, kpaint = (torch.empty((cap, TILE, TILE), device="cuda") for _ in range(2))
    sm = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def outliers():
        L.check(lib.bp_tile_outliers(L.ptr(painted), batch, TILE, std, L.ptr(stats), L.ptr(counts), sm), "tile outliers")

    def keep():
        cursor.zero_()
        L.check(lib.bp_tile_keep(L.ptr(raw), L.ptr(painted), L.ptr(counts), batch, 1, TILE, 0, cap, L.ptr(cursor),
                                 L.ptr(index), L.ptr(kraw), L.ptr(kpaint), sm), "tile keep")

    out = {}
    for name, fn in (("bp_tile_outliers", outliers), ("bp_tile_keep", keep)):
        fn()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(kreps):
                fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) / 1e3 / kreps)
        out[name] = spread(times)
    flagged = int((counts != 0).sum())
    out["flagged_tiles"], out["kept_tiles"] = flagged, min(flagged, cap)
    out["bytes_read_by_outliers"] = 3 * painted.numel() * 4          # sum, squared deviations, count: three passes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kreps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--std", type=float, default=3.0)
    ap.add_argument("--cap", type=int, default=16)
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("outlier_bench needs a GPU")
    pt = make_painter(torch.device("cuda:0"))
    rel, z = TILE / N_PLANE, 0.5
    rng = np.random.Generator(np.random.PCG64(N_PLANE))
    delta = torch.from_numpy((np.exp(rng.standard_normal((N_PLANE, N_PLANE), dtype=np.float32) * 0.5) * 0.05)
                             .astype(np.float32)).cuda()
    out = torch.empty((N_PLANE, N_PLANE), dtype=torch.float64, device="cuda")
    kw = dict(seed=11, batch_size=args.batch, on_device=True, out=out, regularise_std=args.std)
    plain = lambda: LC.paint_plane(pt, delta, rel, TILE, z, **kw)                                       # noqa: E731
    res = {"metric": "paint_plane_report_ms", "tile": TILE, "n_plane": N_PLANE, "batch": args.batch,
           "tiles": len(LC.plane_geometry(N_PLANE, rel, TILE)["origins"]), "regularise_std": args.std, "reps": args.reps}
    plain()                                                                                             # capture + warm-up
    if args.baseline_only:
        res["without_report"] = spread([wall(plain)[0] for _ in range(args.reps)])
        print(json.dumps(res), flush=True)
        return
    report = lambda: LC.paint_plane(pt, delta, rel, TILE, z, return_problematic_tiles=True,            # noqa: E731
                                    max_problematic_tiles=args.cap, **kw)
    rep = report()[1]
    t_plain, t_report = [], []
    for _ in range(args.reps):                                   # alternating: both see the same neighbours
        t_plain.append(wall(plain)[0])
        t_report.append(wall(report)[0])
    res["without_report"], res["with_report"] = spread(t_plain), spread(t_report)
    res["report_adds_ms"] = round(res["with_report"]["median_ms"] - res["without_report"]["median_ms"], 3)
    res["cap"], res["n_problematic"], res["kept"] = args.cap, rep.n_problematic, len(rep.tiles)
    res["kernels_per_batch"] = kernel_times(args.batch, args.std, max(args.cap, 1), args.reps, args.kreps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
