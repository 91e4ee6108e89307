"""Device batch assembly for multi-scale training sets: tiles/s of ``DeviceTileAssembler.get_batch`` against the host
``DataLoader`` path over the same indices, and the training step fed by either, at batches of 64 tiles of 512^2 for
n_scale = 1 (single-scale shift-log chain) and n_scale = 3 (split-scale, step_size = 4, original kept: 4 channels per
field).  Seeded synthetic stacks (2 fields x 2 redshifts x 2 slabs x 2 x 2048^2), ``subtract_minimum`` on, fiducial
architecture, fp32.  One run, timed with HIP events after a warm-up; one JSON line per measurement:

  get_batch      the assembler alone (descriptors on the host, gather [+ minima + pyramid] on the device)
  host_loader    ``DataLoader(Subset(dataset, indices), batch_size)`` alone: SciPy's filters tile by tile
  step           forward + backward + Adam on a resident batch
  step_device    get_batch + step, per batch
  step_host      host loader batch + upload + step, per batch

Usage: python tools/assemble_bench.py [--batch 64] [--batches 8] [--host-batches 1] [--scales 1 3]"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE, N_TILE, STEP, INCLUDE_ORIGINAL = 512, 4, 4, True
REDSHIFTS = [0.0, 0.5]


def make_dataset(n_scale):
    from baryon_painter_amd.utils import data_transforms as T
    from baryon_painter_amd.utils.datasets import BAHAMASDataset
    rng = np.random.Generator(np.random.PCG64(7))
    grid, data = TILE * N_TILE, {}
    for f, amp in (("dm", 5.0e3), ("pressure", 0.05)):
        data[f] = {}
        for z in REDSHIFTS:
            data[f][z] = {slab: np.exp(rng.standard_normal((2, grid, grid), dtype=np.float32)) * np.float32(amp)
                          for slab in ("100", "150")}
            data[f][z].update({"mean_100": amp, "mean_150": amp, "var_100": amp * amp, "var_150": amp * amp})
    fwd, inv = T.create_range_compress_transforms({"dm": 4.0, "pressure": 4}, {"dm": "shift-log", "pressure": "shift-log"})
    if n_scale > 1:
        split, unsplit = T.create_split_scale_transform(n_scale, STEP, INCLUDE_ORIGINAL)
        tr = T.chain_transformations([fwd, T.as_float32, split, T.atleast_3d])
        itr = T.chain_transformations([unsplit, inv, T.squeeze])
        levels = n_scale + int(INCLUDE_ORIGINAL)
    else:
        tr, itr, levels = T.chain_transformations([fwd, T.atleast_3d, T.as_float32]), T.chain_transformations([T.squeeze, inv]), 1
    ds = BAHAMASDataset(data=data, redshifts=REDSHIFTS, label_fields=["pressure"], n_tile=N_TILE, n_stack=2,
                        tile_permutations=True, transform=tr, inverse_transform=itr, n_feature_per_field=levels,
                        scale_to_SLICS=True, subtract_minimum=True, fixed_indexing=True)
    return ds, levels


def timed(fn, reps):
    """ms per call of fn, between two HIP events around `reps` calls (fn has run before: warm)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for r in range(reps):
        fn(r)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--host-batches", type=int, default=1)
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 3])
    args = ap.parse_args()
    from baryon_painter_amd.models import arch as A
    from baryon_painter_amd.optim import FlatAdam
    from baryon_painter_amd.painter import CVAEPainter
    dev, B = "cuda:0", args.batch
    for n_scale in args.scales:
        ds, levels = make_dataset(n_scale)
        common = {"tile": TILE, "batch": B, "n_scale": n_scale, "levels": levels, "subtract_minimum": True}
        rng = np.random.Generator(np.random.PCG64(11))
        batches = [[int(i) for i in rng.integers(0, len(ds), B)] for _ in range(args.batches)]
        torch.manual_seed(1234)
        with contextlib.redirect_stdout(sys.stderr):
            p = CVAEPainter(training_data_set=ds, test_data_set=ds, compute_device=dev,
                            architecture=A.fiducial_architecture(TILE, n_scale=levels))
        p.use_device_assembly()
        asm, model = p.device_assembler, p.model
        model.train(True)
        opt = FlatAdam(model, lr=1e-4)

        def step(x, y, aux):
            elbo = model(x, y, aux)
            opt.zero_grad()
            (-elbo).backward()
            opt.step()

        def report(name, ms, **kw):
            print(json.dumps({"measurement": name, "ms_per_batch": round(ms, 2), "tiles_per_s": round(B / ms * 1e3, 1),
                              **kw, **common}), flush=True)

        x, y, aux = asm.get_batch(batches[0])                                            # warm-up
        assert x.shape == y.shape == (B, levels, TILE, TILE) and bool(torch.isfinite(x).all() & torch.isfinite(y).all())
        step(x, y, aux)
        step(x, y, aux)
        ms_asm = timed(lambda r: asm.get_batch(batches[r % len(batches)]), args.batches)
        report("get_batch", ms_asm)
        ms_step = timed(lambda r: step(x, y, aux), args.batches)
        report("step", ms_step)

        def device_step(r):
            step(*asm.get_batch(batches[r % len(batches)]))
        ms_dev = timed(device_step, args.batches)
        report("step_device", ms_dev, assembler_share=round(1 - ms_step / ms_dev, 3))

        host_idx = [i for b in batches[:args.host_batches] for i in b]
        loader = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, host_idx), batch_size=B, shuffle=False)
        ms_host = timed(lambda r: [None for _ in loader], 1) / args.host_batches
        report("host_loader", ms_host)

        def host_steps(r):
            for fields, _, z in loader:
                step(torch.cat(fields[1:], dim=1).to(dev), fields[0].to(dev), z.to(device=dev, dtype=torch.float32))
        ms_hs = timed(host_steps, 1) / args.host_batches
        report("step_host", ms_hs, loader_share=round(1 - ms_step / ms_hs, 3))
        del p, asm, model, opt, x, y, aux
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
