"""What painting a second label field costs: fiducial CVAE on 512^2 tiles in batches of 64, synthetic weights and
statistics, all in one run.  One JSON line per measurement:

  paint_stream_fields   raw host tiles in, (N, 2, H, W) physical host tiles out: a 2-field painter (pressure
                        "shift-log-2p", gas "log") through the device pipeline (bp_paint_store_fields behind the graph)
  paint_stream_single   the single-field painter (pressure alone) on the same tiles, in the same run; the two are timed
                        alternately, ``--repeats`` times each, and every repeat is reported
  store_fields          bp_paint_store_fields on an F-channel head of one batch against F launches of
                        bp_paint_store_mode on its channel-slice views: the two alternate for ``--rounds`` rounds of
                        ``--launches`` launches between two device events; every round and the medians are reported

No figure is fixed in advance.  Usage: python tools/fields_bench.py [--tiles 256] [--batch 64] [--tile 512]
[--repeats 3] [--launches 400] [--rounds 5] [--fields 2]"""
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

MODES = {"dm": "log", "pressure": "shift-log-2p", "gas": "log"}
K_VALUES = {"dm": 2.0, "pressure": (0.5, 3.0), "gas": 2.5}


def make_painter(dev, tile, labels):
    from baryon_painter_amd.models import arch as A
    from baryon_painter_amd.models.cvae import CVAE
    from baryon_painter_amd.painter import CVAEPainter
    from baryon_painter_amd.utils import data_transforms as T
    from baryon_painter_amd.utils.datasets import SyntheticTileDataset, compile_transform
    ds = SyntheticTileDataset(n_sample=8, tile_size=tile, seed=3)
    stats = dict(ds.stats)
    stats["gas"] = {z: {"mean": 2.0 * s["mean"], "var": 3.0 * s["var"]} for z, s in ds.stats["pressure"].items()}
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(sys.stderr):
        model = CVAE(A.fiducial_architecture(tile, n_fields=len(labels)), dev)
    model.train(False)
    pt = CVAEPainter.__new__(CVAEPainter)
    pt.model, pt.compute_device, pt.sync, pt.dtype = model, dev, None, "f32"
    pt.input_field, pt.label_fields = ds.input_field, list(labels)
    fwd, inv = T.create_range_compress_transforms(K_VALUES, MODES)
    pt.transform = compile_transform(T.chain_transformations([fwd, T.atleast_3d, T.as_float32]), stats)
    pt.inverse_transform = compile_transform(T.chain_transformations([T.squeeze, inv]), stats)
    return pt, ds


def tiles_of(ds, n):
    raw = np.stack([ds.raw_fields(i)[0] for i in range(8)])
    zs = np.array([ds.raw_fields(i)[2] for i in range(8)])
    reps = (n + 7) // 8
    return np.tile(raw, (reps, 1, 1))[:n], np.tile(zs, reps)[:n]


def stream_time(pt, tin, zs, batch, tout):
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pt.paint_stream(tin, zs, batch_size=batch, out=tout)
        torch.cuda.synchronize()
        return time.perf_counter() - t0


def store_times(F, n, tile, launches, rounds):
    """(ms per bp_paint_store_fields launch, ms per F bp_paint_store_mode launches) on an (n, tile, tile, F) head: one
    figure per round, each the mean over ``launches`` launches between two events."""
    from baryon_painter_amd import _lib as L
    lib = L.load()
    modes = [(2, 1, 0, 3, 4, 5)[j % 6] for j in range(F)]
    head = torch.rand((n, tile, tile, F), device="cuda") * 0.9
    view = L.View(head.data_ptr(), n, tile, tile, F, F, 0)
    rec = torch.rand((n, F, 4), dtype=torch.float64, device="cuda") + 0.5
    recs = [rec[:, j].contiguous() for j in range(F)]
    dst = torch.empty((n, F, tile, tile), device="cuda")
    dsts = [torch.empty((n, 1, tile, tile), device="cuda") for _ in range(F)]
    views = [L.View(head.data_ptr(), n, tile, tile, 1, F, j) for j in range(F)]
    arr = (C.c_int32 * F)(*modes)
    sm = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fields():
        L.check(lib.bp_paint_store_fields(arr, F, 1, 0, C.byref(view), None, 1, L.ptr(rec), L.ptr(dst), sm), "fields")

    def slices():
        for j in range(F):
            L.check(lib.bp_paint_store_mode(modes[j], C.byref(views[j]), None, 1, L.ptr(recs[j]), L.ptr(dsts[j]), sm),
                    "slice")
    times = {fields: [], slices: []}
    for fn in (fields, slices):                                  # first launches
        for _ in range(5):
            fn()
    for _ in range(rounds):                                      # the two alternate: clocks and neighbours drift
        for fn in (fields, slices):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[fn].append(a.elapsed_time(b) / launches)
    for j in range(F):                                           # what is timed computes the same bits
        assert torch.equal(torch.nan_to_num(dst[:, j], nan=-7.0), torch.nan_to_num(dsts[j][:, 0], nan=-7.0)), j
    return times[fields], times[slices]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fields", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fields_bench.py measures on a GPU: none found")
    dev = "cuda:0"
    common = {"tile": args.tile, "batch": args.batch}
    both, ds = make_painter(dev, args.tile, ("pressure", "gas"))
    single, _ = make_painter(dev, args.tile, ("pressure",))
    assert both.can_paint_stream() and single.can_paint_stream()
    raw, zs = tiles_of(ds, args.tiles)
    tin = torch.from_numpy(raw).pin_memory()
    out2 = torch.empty((len(raw), 2, args.tile, args.tile), dtype=torch.float32).pin_memory()
    out1 = torch.empty(raw.shape, dtype=torch.float32).pin_memory()
    warm = 2 * args.batch
    for pt, out in ((both, out2), (single, out1)):               # capture, page-lock, first launches
        stream_time(pt, tin[:warm], zs[:warm], args.batch, out[:warm])
    for r in range(args.repeats):
        for name, pt, out in (("paint_stream_fields", both, out2), ("paint_stream_single", single, out1)):
            dt = stream_time(pt, tin, zs, args.batch, out)
            print(json.dumps({"measurement": name, "repeat": r, "label_fields": pt.label_fields, "tiles": len(raw),
                              "tiles_per_s": round(len(raw) / dt, 1),
                              "ms_per_batch": round(dt / (len(raw) / args.batch) * 1e3, 2), **common}), flush=True)
    for pt in (both, single):
        pt.release_paint_buffers()
    del both, single, out1, out2
    torch.cuda.empty_cache()
    ms_fields, ms_slices = store_times(args.fields, args.batch, args.tile, args.launches, args.rounds)
    print(json.dumps({"measurement": "store_fields", "fields": args.fields, "launches_per_round": args.launches,
                      "ms_store_fields": [round(v, 4) for v in ms_fields],
                      "ms_store_mode_x_fields": [round(v, 4) for v in ms_slices],
                      "median_ms": [round(float(np.median(ms_fields)), 4), round(float(np.median(ms_slices)), 4)],
                      **common}))


if __name__ == "__main__":
    main()
