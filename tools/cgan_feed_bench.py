"""What feeds ``CGANPainter.train``: the host loop, the device assembler, and tensors that are already resident, at the
fiducial geometry (tile 512, nine blocks), in ONE process.

    python tools/cgan_feed_bench.py [--batches 6 64] [--dtypes fp32 bf16] [--repeats 5] [--iters 2] [--json PATH]

Per trunk dtype and batch size, after a warm-up of every variant, REPEATS rounds; a round times ITERS training iterations
of each variant in turn (host clock around work that ends in a device synchronise), so drifts of the machine fall on all
variants alike:

    host       ``CGANPainter.train`` as it was: tiles cut, permuted, added and transformed in NumPy, uploaded, copied
    assembler  ``CGANPainter.train`` after ``use_device_assembly()``: one bp_gather_tiles_gan launch per iteration
    resident   ``CGAN.train_step`` on device tensors, the floor tools/cgan_train_bench.py measures

Then, alone, with device events (warm-up, median of REPEATS rounds): bp_gather_tiles_gan with the bytes it moves, and what
it replaces on the same samples -- the layout glue of ``train_step`` on resident tensors (one copy and four
bp_nchw_to_view launches), and the existing kernels' composition from the same descriptors (two bp_gather_tiles, two
bp_paint_load_cam, then that glue).  Medians and ranges are printed, and one JSON line at the end.  The training set is
seeded random slab stacks (2 redshifts x 2 slabs x 2 x 2048^2 per field).  Needs a GPU: there is no fallback."""
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
from baryon_painter_amd.painter import CGANPainter                  # noqa: E402
from baryon_painter_amd.utils.datasets import BAHAMASDataset        # noqa: E402

TILE, N_RES, N_TILE = 512, 9, 4
REDSHIFTS = [0.0, 0.5]
HBM_TB_S = 6.3


def stat(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def training_set(tile):
    grid = tile * N_TILE
    rng = np.random.Generator(np.random.PCG64(5))
    data = {}
    for f, amp in (("dm", 5.0e3), ("pressure", 0.05)):
        data[f] = {z: {"100": rng.random((2, grid, grid), dtype=np.float32) * amp + 0.01 * amp,
                       "150": rng.random((2, grid, grid), dtype=np.float32) * amp + 0.02 * amp,
                       "mean_100": 0.5 * amp, "mean_150": 0.5 * amp, "var_100": amp * amp / 12, "var_150": amp * amp / 12}
                   for z in REDSHIFTS}
    return BAHAMASDataset(data=data, redshifts=REDSHIFTS, label_fields=["pressure"], n_tile=N_TILE, tile_permutations=True,
                          scale_to_SLICS=True, fixed_indexing=True)


def events(fn, repeats, rep):
    """us per call: ``repeats`` rounds of ``rep`` calls between two events, after two warm-up rounds."""
    out = []
    for r in range(repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rep):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            out.append(e0.elapsed_time(e1) * 1e3 / rep)
    return out


def iterations(p, asm, batch, repeats, iters):
    """ms per iteration of the three feeds, interleaved."""
    ds, m = p.training_data, p.model
    idx = np.random.default_rng(1).integers(0, len(ds), batch)
    raw = [CGANPainter._raw(ds, int(i)) for i in idx]
    x = torch.from_numpy(np.stack([p.transform(r[1], "pressure", r[2])[None] for r in raw])).cuda()
    y = torch.from_numpy(np.stack([p.transform(r[0], "dm", r[2])[None] for r in raw])).cuda()
    z = torch.tensor([r[2] for r in raw], dtype=torch.float32).cuda()
    opts = (torch.optim.Adam(m.g_parameters(), lr=5e-5, betas=(0.5, 0.999)),
            torch.optim.Adam(m.d_parameters(), lr=5e-5, betas=(0.5, 0.999)))

    def host(k):
        p.device_assembler = None
        p.train(n_iter=k, batch_size=batch)

    def assembler(k):
        p.device_assembler = asm
        p.train(n_iter=k, batch_size=batch)

    def resident(k):
        m.train(True)
        for _ in range(k):
            m.train_step(x, y, z, *opts)
    variants = [("host", host), ("assembler", assembler), ("resident", resident)]
    times = {v[0]: [] for v in variants}
    for r in range(repeats + 1):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(iters)
            torch.cuda.synchronize()
            if r:                                       # (round 0: the warm-up of every variant)
                times[name].append((time.perf_counter() - t0) * 1e3 / iters)
    p.device_assembler = asm
    return {k: stat(v) for k, v in times.items()}, (x, y, z, idx)


def kernels_alone(p, asm, batch, repeats, resident):
    """us per call of the gather and of what it replaces, into the training plan's own buffers."""
    lib, ds, m, t = L.load(), p.training_data, p.model, TILE
    x, y, z, idx = resident
    plan = m._plan(batch)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cam, aux = p._cam_rows([ds.sample_idx_to_redshift(int(i)) for i in idx])
    layout, nbytes = asm._gan_block(idx, cam, aux)
    host = np.zeros(nbytes, np.uint8)
    for off, a in layout.values():
        host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
    block = torch.from_numpy(host).cuda()
    q = {k: C.c_void_p(block.data_ptr() + off) for k, (off, _) in layout.items()}

    def gather():
        plan.fill(lambda g, r, f, xn: L.check(lib.bp_gather_tiles_gan(
            q["in100"], q["in150"], q["in_xf"], None, q["lab100"], q["lab150"], q["lab_xf"], q["cam"], q["aux"], batch, t,
            C.byref(g), C.byref(r), C.byref(f), L.ptr(xn), st), "gather"))
    zc = (z - 1.0).reshape(batch, 1).contiguous()

    def glue():
        plan._keep = (y.contiguous(), zc)
        L.check(lib.bp_nchw_to_view(L.ptr(y), 1, L.ptr(zc), 1, C.byref(plan.y2.view), st), "generator input")
        plan.load_real(x)
    raw = [torch.empty((batch, 1, t, t), device="cuda") for _ in range(2)]
    out = [torch.empty((batch, 1, t, t), device="cuda") for _ in range(2)]
    camd = [torch.from_numpy(np.ascontiguousarray(cam[:, k])).cuda() for k in range(2)]      # (n, 3) rows per field
    dense = [L.View(o.data_ptr(), batch, t, t, 1, 1, 0) for o in out]

    def composition():
        for k, (a, b, xf) in enumerate((("in100", "in150", "in_xf"), ("lab100", "lab150", "lab_xf"))):
            L.check(lib.bp_gather_tiles(q[a], q[b], q[xf], batch, t, L.ptr(raw[k]), st), "gather tiles")
            L.check(lib.bp_paint_load_cam(L.ptr(raw[k]), 1, L.ptr(camd[k]), None, 0,
                                          C.byref(dense[k]), st), "load cam")
        glue()
    px = float(batch) * t * t
    moved = 48.0 * px                                   # 4 stack reads; 2 + 3 + 2 + 1 floats stored per pixel
    res = {}
    for name, fn in (("bp_gather_tiles_gan", gather), ("layout glue of train_step", glue),
                     ("existing kernels' composition", composition)):
        res[name] = stat(events(fn, repeats, 10))
    g = res["bp_gather_tiles_gan"]
    g["bytes"] = moved
    g["tb_per_s"] = moved / g["median"] / 1e6
    g["share_of_hbm"] = g["tb_per_s"] / HBM_TB_S
    g["ns_per_pixel"] = g["median"] * 1e3 / px
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[6, 64])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("at least five repeats")
    if not torch.cuda.is_available():
        raise SystemExit("cgan_feed_bench needs a GPU")
    ds = training_set(TILE)
    result = {"tile": TILE, "n_res": N_RES, "repeats": a.repeats, "iters": a.iters, "device": torch.cuda.get_device_name(0),
              "runs": {}}
    asm = None
    for batch in a.batches:
        for dtype in a.dtypes:
            torch.manual_seed(0)
            p = CGANPainter(training_data_set=ds, tile_size=TILE, compute_device="cuda:0", n_res=N_RES, train_dtype=dtype)
            if asm is None:
                p.use_device_assembly()                 # the stacks go up once; every painter shares them
                asm = p.device_assembler
            it, resident = iterations(p, asm, batch, a.repeats, a.iters)
            alone = kernels_alone(p, asm, batch, a.repeats, resident)
            g = alone["bp_gather_tiles_gan"]
            floor, fed = it["resident"], it["assembler"]
            row = {"iteration_ms": it, "tiles_per_s": {k: batch / v["median"] * 1e3 for k, v in it.items()},
                   "alone_us": alone, "host_over_assembler": it["host"]["median"] / fed["median"],
                   "assembler_minus_resident_ms": fed["median"] - floor["median"],
                   "resident_scatter_ms": floor["max"] - floor["min"],
                   "claim_holds": bool(fed["median"] <= floor["median"] + g["median"] / 1e3 + (floor["max"] - floor["min"]))}
            result["runs"][f"{dtype}/{batch}"] = row
            print(f"{dtype} trunk, batch {batch}: tile {TILE}, {N_RES} blocks; median [min, max] over {a.repeats} rounds of "
                  f"{a.iters} iterations")
            for k, v in it.items():
                print(f"  fed by {k:10s} {v['median']:9.2f} ms [{v['min']:.2f}, {v['max']:.2f}]  "
                      f"{row['tiles_per_s'][k]:8.1f} tiles/s")
            print(f"  host / assembler {row['host_over_assembler']:.2f} x; assembler - resident "
                  f"{row['assembler_minus_resident_ms']:+.3f} ms; the gather alone {g['median'] / 1e3:.3f} ms; scatter of "
                  f"the resident figure {row['resident_scatter_ms']:.3f} ms; claim holds: {row['claim_holds']}")
            for k, v in alone.items():
                print(f"  {k:32s} {v['median']:9.1f} us [{v['min']:.1f}, {v['max']:.1f}]")
            print(f"    the gather moves {g['bytes'] / 1e6:.1f} MB: {g['tb_per_s']:.3f} TB/s, {100 * g['share_of_hbm']:.1f} % of "
                  f"{HBM_TB_S} TB/s; {g['ns_per_pixel']:.4f} ns per pixel", flush=True)
            del p, resident
            gc.collect()                                # (a model and its plans reference each other)
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
