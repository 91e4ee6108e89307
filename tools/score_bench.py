"""What scoring costs: a two-head fiducial CVAE (``fiducial_architecture(predict_var=True)``) on 512^2 tiles in batches
of 64 generator samples, synthetic weights and statistics, all in one process.  One JSON line per measurement:

  loglik_samples   bp_loglik_samples alone on the two heads of one batch (K draws of 64 / K tiles, one channel) beside
                   bp_loglik_forward on the same heads.  The two alternate for ``--rounds`` rounds of ``--launches``
                   launches between two device events; every round, the medians, and the bytes each MUST move (x, mu
                   and var read once; bp_loglik_forward also writes x_mu and x_log_var) with the GB/s they come to.
                   ``buffers: "rotating"``: every launch takes the next of ``--sets`` head pairs, more bytes together
                   than the 256 MiB of last-level cache, so the heads come from HBM; ``buffers: "same"``: one pair,
                   134 MB, launched again and again -- cache-resident, an upper bound and not what a batch sees
  posterior_score  bp_posterior_score alone on 64 / K tiles of a (1, 16, 16) latent (cache-resident: 100 KB)
  model_score      ``CVAE.score`` on one device-resident batch: ``wall_ms`` (host clock around a synchronised call),
                   ``device_ms`` (two events around the call's launches) and ``enqueue_ms`` (the host clock until the
                   call has issued its last launch).  The time of a batch spent outside kernels is wall_ms minus the sum
                   of the kernel times of a kernel trace of this measurement (``--only model``), which this tool does
                   not take itself
  painter_score    raw host tiles and truths in, five columns out: ``CVAEPainter.score(draws=K)``, every repeat

No figure is fixed in advance.  Usage: python tools/score_bench.py [--tiles 32] [--batch 64] [--tile 512]
[--draws 1,4,16] [--repeats 3] [--launches 50] [--rounds 5] [--sets 4] [--only kernels|model|painter]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pixel_noise_bench import make_painter  # noqa: E402


def _rounds(fns, launches, rounds):
    """ms per launch of each of ``fns``, one figure per round; the functions alternate (clocks and neighbours drift)."""
    times = {fn: [] for fn in fns}
    for fn in fns:
        for _ in range(5):
            fn()
    for _ in range(rounds):
        for fn in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[fn].append(a.elapsed_time(b) / launches)
    return [times[fn] for fn in fns]


def loglik_times(K, batch, tile, launches, rounds, sets):
    from baryon_painter_amd import _lib as L
    lib = L.load()
    n = batch // K
    sm = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.rand((n, 1, tile, tile), device="cuda")
    heads = [(torch.randn((batch, tile, tile, 1), device="cuda"), torch.randn((batch, tile, tile, 1), device="cuda") - 4.0)
             for _ in range(sets)]
    views = [tuple(L.View(t.data_ptr(), batch, tile, tile, 1, 1, 0) for t in pair) for pair in heads]
    ll = L.Loglik(n, K, 1, tile, tile, 1, 1, 1.0, 1.0, 1.0)
    ws = torch.zeros(max(lib.bp_loglik_samples_workspace(C.byref(ll)), lib.bp_loglik_workspace(C.byref(ll))) // 8 + 32,
                     dtype=torch.float64, device="cuda")
    out = torch.zeros((batch, 1), dtype=torch.float64, device="cuda")
    x_mu, x_lv = torch.empty((batch, 1, tile, tile), device="cuda"), torch.empty((batch, 1, tile, tile), device="cuda")
    stats = torch.zeros(5, device="cuda")
    turn = {"s": 0, "f": 0}

    def samples(step=1):
        mu, var = views[turn["s"] % sets]
        turn["s"] += step
        L.check(lib.bp_loglik_samples(C.byref(ll), L.ptr(x), C.byref(mu), C.byref(var), L.ptr(out), L.ptr(ws),
                                      ws.numel() * 8, sm), "loglik samples")

    def forward(step=1):
        mu, var = views[turn["f"] % sets]
        turn["f"] += step
        L.check(lib.bp_loglik_forward(C.byref(ll), L.ptr(x), C.byref(mu), C.byref(var), None, L.ptr(x_mu), L.ptr(x_lv),
                                      L.ptr(stats), L.ptr(ws), ws.numel() * 8, sm), "loglik forward")
    px = batch * tile * tile
    must = [4 * (2 * px + px // K), 4 * (4 * px + px // K)]
    res = []
    for name, fns in (("rotating", (samples, forward)), ("same", (lambda: samples(0), lambda: forward(0)))):
        ms_s, ms_f = _rounds(fns, launches, rounds)
        med = [float(np.median(ms_s)), float(np.median(ms_f))]
        res.append({"measurement": "loglik_samples", "buffers": name, "sets": sets if name == "rotating" else 1,
                    "draws": K, "launches_per_round": launches, "ms_loglik_samples": [round(v, 4) for v in ms_s],
                    "ms_loglik_forward": [round(v, 4) for v in ms_f], "median_ms": [round(v, 4) for v in med],
                    "bytes": must, "GB_per_s": [round(b / (m * 1e-3) / 1e9, 1) for b, m in zip(must, med)]})
    # the two kernels agree on the batch mean of the free-variance term (the loss keeps -log(2 pi)/2 once)
    turn["s"] = turn["f"] = 0
    samples(0)
    forward(0)
    torch.cuda.synchronize()
    c0 = -0.5 * np.log(2 * np.pi)
    assert abs(float(out.mean()) - ((float(stats[4]) - c0) + tile * tile * c0)) <= 2e-5 * abs(float(out.mean()))
    return res


def posterior_times(K, batch, launches, rounds, dim_z=(1, 16, 16)):
    from baryon_painter_amd import _lib as L
    lib = L.load()
    n = batch // K
    sm = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lt = L.Latent(n, K, *dim_z, 1e-7)
    st = torch.randn((4, n, *dim_z), device="cuda")
    eps = torch.randn((K, n, *dim_z), device="cuda")
    ll = torch.randn((K * n, 1), dtype=torch.float64, device="cuda") * 30 - 4e4
    out = torch.zeros((n, 5), dtype=torch.float64, device="cuda")

    def score():
        L.check(lib.bp_posterior_score(C.byref(lt), L.ptr(st), L.ptr(eps), L.ptr(ll), 1, L.ptr(out), None, sm), "score")
    ms, = _rounds((score,), launches, rounds)
    return {"measurement": "posterior_score", "draws": K, "tiles": n, "dim_z": list(dim_z), "launches_per_round": launches,
            "ms": [round(v, 4) for v in ms], "median_ms": round(float(np.median(ms)), 4)}


def model_times(model, K, batch, tile, repeats):
    n = batch // K
    x = torch.rand((n, 1, tile, tile), device="cuda")
    y = torch.rand((n, 1, tile, tile), device="cuda")
    aux = torch.full((n,), 0.5, device="cuda")
    eps = torch.randn((K, n, *model.dim_z), device="cuda")
    for _ in range(2):
        model.score(x, y, aux, draws=K, eps=eps)
    wall, dev, enq = [], [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = model.score(x, y, aux, draws=K, eps=eps)
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        wall.append((t2 - t0) * 1e3)
        enq.append((t1 - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    assert bool(torch.isfinite(out[:, :4]).all())
    r = lambda v: [round(t, 3) for t in v]                                            # noqa: E731
    return {"measurement": "model_score", "draws": K, "tiles": n, "wall_ms": r(wall), "device_ms": r(dev),
            "enqueue_ms": r(enq), "median_wall_ms": round(float(np.median(wall)), 3),
            "tiles_per_s": round(n / (float(np.median(wall)) * 1e-3), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=32)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--draws", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--only", choices=["kernels", "model", "painter"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench.py measures on a GPU: none found")
    draws = [int(k) for k in args.draws.split(",")]
    common = {"tile": args.tile, "batch": args.batch}
    if args.only in (None, "kernels"):
        for K in draws:
            for res in loglik_times(K, args.batch, args.tile, args.launches, args.rounds, args.sets):
                print(json.dumps({**res, **common}), flush=True)
            torch.cuda.empty_cache()
            print(json.dumps({**posterior_times(K, args.batch, args.launches, args.rounds), **common}), flush=True)
    if args.only == "kernels":
        return
    pt, ds = make_painter("cuda:0", args.tile)
    if args.only in (None, "model"):
        for K in draws:
            print(json.dumps({**model_times(pt.model, K, args.batch, args.tile, max(args.repeats, 5)), **common}),
                  flush=True)
    if args.only == "model":
        return
    fields = [ds.raw_fields(i) for i in range(8)]
    reps = (args.tiles + 7) // 8
    raw = np.tile(np.stack([f[0] for f in fields]), (reps, 1, 1))[:args.tiles]
    truth = np.tile(np.stack([f[1] for f in fields]), (reps, 1, 1))[:args.tiles]
    zs = np.tile(np.array([f[2] for f in fields]), reps)[:args.tiles]
    for K in draws:
        m = min(len(raw), 2 * args.batch // K)
        pt.score(raw[:m], truth[:m], zs[:m], draws=K, batch_size=args.batch, seed=5)      # plans, first launches
        for r in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = pt.score(raw, truth, zs, draws=K, batch_size=args.batch, seed=5)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert np.isfinite(d["bound"]).all()
            print(json.dumps({"measurement": "painter_score", "draws": K, "repeat": r, "tiles": len(raw),
                              "seconds": round(dt, 4), "tiles_per_s": round(len(raw) / dt, 2),
                              "mean_bound": round(float(d["bound"].mean()), 3),
                              "mean_ess": round(float(d["ess"].mean()), 3), **common}), flush=True)


if __name__ == "__main__":
    main()
