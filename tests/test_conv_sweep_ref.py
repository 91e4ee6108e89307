"""CPU: the convolution sweep's cases and reference (tests/conv_sweep.py), and which kernels the dispatcher picks for them.

* reference() -- oracle.ops in float64 -- against torch.nn.functional.conv2d / conv_transpose2d and their autograd in
  float64 at every case: the NumPy oracle is pinned to the reference project's goldens at the model's layers only, the
  sweep adds k < stride, pad >= k, out_pad, 1 x 1 tensors and channel counts off every grid.
* the case list is deterministic, covers every grid cell, and every gate / neighbour sits where conv_sweep.GATES says.
* bp_conv_kernel_id is host-only arithmetic: the table of ids over the sweep must reach every kernel family, chunk
  width, channel-block shape and pixel packing of the dispatcher (run with -s to see the table).
"""
import collections
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from baryon_painter_amd import _lib as L

import conv_sweep as S


def _torch4(case, xa, w, bias, dy):
    tr, ci, co, k, s, p, op = case[:7]
    xt = torch.from_numpy(xa).requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    bt = None if bias is None else torch.from_numpy(np.asarray(bias, np.float64)).requires_grad_(True)
    y = F.conv_transpose2d(xt, wt, bt, s, p, op) if tr else F.conv2d(xt, wt, bt, s, p)
    y.backward(torch.from_numpy(dy))
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), None if bt is None else bt.grad.numpy()


def test_reference_equals_torch_float64():
    worst = (0.0, "")
    for i, (tag, case) in enumerate(S.tagged_cases()):
        x, w, bias, dy, pw = S.make_inputs(case, i, with_bias=i % 3 == 0)
        got = S.reference(case, x, w, bias, dy, pw)
        xa = S.activated(x, pw)
        want = _torch4(case, xa, w.astype(np.float64), bias, dy.astype(np.float64))
        assert got[0].shape[2:] == S.out_shape(case)
        for name, a, b in zip(("y", "dx", "dw", "dbias"), got, want):
            if b is None:
                b = dy.astype(np.float64).sum(axis=(0, 2, 3))
            assert a.shape == b.shape, (tag, case, name)
            err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
            worst = max(worst, (err, S.case_id(tag, case) + "/" + name))
            assert err <= 1e-12, (S.case_id(tag, case), name, err)
    print("\nworst deviation of oracle.ops from torch float64: %.2e at %s" % worst)


def test_bound_and_terms_are_the_reference_of_the_magnitudes():
    """bound() dominates |reference()| elementwise; terms() counts the products: with all-ones operands the
    reference itself is the count, and an element without a product is exactly the bias / zero."""
    for i, (tag, case) in list(enumerate(S.tagged_cases()))[::37]:
        x, w, bias, dy, pw = S.make_inputs(case, i, with_bias=True)
        ref, bnd, T = S.reference(case, x, w, bias, dy, pw), S.bound(case, x, w, bias, dy, pw), S.terms(case)
        for r, b, t in zip(ref, bnd, T):
            assert (np.abs(r) <= b * (1 + 1e-12)).all(), tag
            assert np.broadcast_shapes(t.shape, r.shape) == r.shape and (t >= 0).all() and (t == np.round(t)).all()
        nobody = np.broadcast_to(T[0], ref[0].shape) == 0
        assert (ref[0][nobody] == np.broadcast_to(bias[None, :, None, None].astype(np.float64), ref[0].shape)[nobody]).all()
        assert (ref[1][np.broadcast_to(T[1], ref[1].shape) == 0] == 0).all()
    # k < stride: three of the four phases of this layer have no tap at all
    case = dict(S.EXTRA)["taps:T_k1s2"]
    assert (S.terms(case)[0] == 0).mean() > 0.7
    # trailing rows that no output reads
    case = dict(S.EXTRA)["ext:trailing_s3"]
    assert (S.terms(case)[1][0, 0, -2:, :] == 0).all() and (S.terms(case)[1][0, 0, :-2, :-2] > 0).all()


def test_bf16_rounding_is_torch_s():
    rng = np.random.Generator(np.random.PCG64(3))
    a = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 20, 100000))).astype(np.float32)
    a[:4] = [0.0, -0.0, 1.00390625, 1.01171875]                   # two exact ties: to even
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(S.bf16_round(a), want)


def test_cases_are_deterministic_and_cover_the_grid():
    a, b = S.tagged_cases(), S.tagged_cases()
    assert a == b and S.checksum(S.cases()) == S.checksum([c for _, c in b])
    assert len({t for t, _ in a}) == len(a), "tags are unique"
    assert all(S.valid(c) for _, c in a)
    cells = S.grid_cells()
    assert len(cells) == 504 and len(set(cells)) == 504
    grid = S.grid_cases()
    assert [(c[0], c[3], c[4], c[5], c[6]) for c in grid] == cells, "every grid cell present, none dropped"
    for k in S.KS:
        assert {c[5] for c in grid if c[3] == k} == {0, (k - 1) // 2, k // 2, k - 1, k + 1}
    for c in S.cases():
        tr, ci, co, k, s, p, op, n, h, w = c
        ho, wo = S.out_shape(c)
        assert n <= S.MAX_N and h <= S.MAX_H and w <= S.MAX_W and max(ci, co) <= 130, c
        assert ho <= 4 * S.MAX_H + 12 and wo <= 4 * S.MAX_W + 12, c
    assert {c[1] for c in grid} | {c[2] for c in grid} == set(S.CHANNELS), "every channel count of the set is drawn"
    # pinned: a change of the generator is a change of what the GPU sweep runs, and shows here
    assert (len(a), S.checksum(S.cases())) == (PINNED_LEN, PINNED_SUM), (len(a), hex(S.checksum(S.cases())))


PINNED_LEN, PINNED_SUM = 753, 0x36793850F545E9F0


def _ids(lib, conv):
    cv = L.Conv(*conv[:7])
    return [lib.bp_conv_kernel_id(C.byref(cv), d) for d in (L.PACK_FWD, L.PACK_BWD)]


def test_gates_and_neighbours_sit_where_the_case_list_says():
    lib = L.load()
    for name, conv, fams, inside in S.GATES:
        base = [S.family(i) for i in _ids(lib, conv)]
        for d in (0, 1):
            if fams[d] is None:
                continue
            assert base[d] == fams[d], (name, d, base)
            outside = 0
            for f in S.NEIGHBOUR_FIELDS:
                nb = S.neighbour(conv, f)
                if nb is None:
                    assert f not in inside[d], (name, f)
                    continue
                same = S.family(_ids(lib, nb)[d]) == fams[d]
                assert same == (f in inside[d]), "%s %s (direction %d): %s the gate" % (name, f, d, "inside" if same else "outside")
                outside += not same
            assert outside >= 2, name
    tags = {t for t, _ in S.tagged_cases()}
    for name, conv, _, _ in S.GATES:
        assert "gate:" + name in tags and "gate:" + name + ":ragged" in tags
        for f in S.NEIGHBOUR_FIELDS:
            assert (S.neighbour(conv, f) is None) or ("near:%s:%s" % (name, f)) in tags


def test_hand_picked_cases_sit_on_the_kernels_their_comments_name():
    lib = L.load()
    assert set(S.EXTRA_IDS) == {t for t, _ in S.EXTRA}
    for tag, case in S.EXTRA:
        ids = tuple(_ids(lib, case))
        assert ids == S.EXTRA_IDS[tag], (tag, ids)
        fams = {S.family(i) for i in ids}
        kind = tag.split(":")[0]
        if kind == "wide":
            assert fams <= {"dma4", "dma8", "dmaf", "plain-mt4"} and fams & {"dma4", "dma8", "dmaf"}, (tag, fams)
        if kind in ("wres", "small", "tiny"):
            assert kind in fams, (tag, fams)
        if kind in ("chan", "cop"):
            assert fams <= {"plain-mt4", "plain-mt1", "dma4", "dma8", "dmaf"}, (tag, fams)
    # the chunk widths the "chan" comments name: cin 17 / 33 -> 16 with a one-channel tail, 9 -> 8, 5 -> 8 (cin4 = 8)
    for tag, cc in (("chan:17_16_k3", 16), ("chan:33_65_k3", 16), ("chan:9_33_k3", 8), ("chan:5_17_k3", 8)):
        assert S.igemm_shape(S.EXTRA_IDS[tag][0])[0] == cc, tag


# bp_conv_kernel_id (forward, data gradient) and bp_conv_bf16_packed_elems (forward, data gradient) of every
# convolution of arch.fiducial_architecture (with and without predict_var), of the CGAN generator and of its
# discriminator, as the commit before the sweep computed them: the sources that compute the fp32 ids are untouched by the
# fixes the sweep brought (conv_wgrad.hip's entry into its chunked / general kernels, b_config's persistent form), and the
# bf16 image of no model layer may change size with them.
MODEL_LAYER_IDS = {
    (0, 2, 8, 4, 2, 1, 0): (780002, 8114, 4096, 4096),
    (0, 8, 16, 8, 4, 2, 0): (760000, 770000, -1, 16384),
    (0, 16, 32, 8, 4, 2, 0): (8211, 316114, -1, 32768),
    (0, 32, 2, 5, 1, 2, 0): (316114, 4214, 12800, 5120),
    (0, 1, 8, 4, 2, 1, 0): (780001, 8114, 4096, 4096),
    (0, 64, 2, 5, 1, 2, 0): (316114, 4414, 25600, 10240),
    (1, 1, 1, 4, 2, 1, 0): (842111, 842110, 4096, 4096),
    (1, 1, 1, 8, 4, 2, 0): (884111, 884110, 16384, -1),
    (0, 3, 16, 5, 1, 2, 0): (700000, 8114, 5120, 19968),
    (0, 16, 32, 4, 2, 1, 0): (416212, 720000, 16384, 16384),
    (0, 32, 64, 4, 2, 1, 0): (730000, 740000, 65536, 65536),
    (0, 64, 128, 4, 2, 1, 0): (108424, 116414, 262144, 262144),
    (0, 128, 128, 3, 1, 1, 0): (216424, 216424, 294912, 294912),
    (1, 128, 64, 4, 2, 1, 0): (116414, 108424, 262144, 262144),
    (1, 64, 32, 4, 2, 1, 0): (740000, 730000, 65536, 65536),
    (1, 32, 16, 4, 2, 1, 0): (720000, 416212, 16384, 16384),
    (0, 16, 8, 7, 1, 3, 0): (750000, 710000, 30720, 14336),
    (0, 8, 1, 5, 1, 2, 0): (905081, 905018, 13312, 3584),
    (0, 1, 1, 3, 1, 1, 0): (903011, 903011, 1536, 1536),
    (0, 2, 32, 9, 1, 4, 0): (4214, 909322, 18432, 41472),
    (0, 32, 64, 3, 2, 1, 0): (8414, 316214, 18432, 32768),
    (0, 64, 128, 3, 2, 1, 0): (108424, 116414, 73728, 131072),
    (1, 128, 64, 3, 2, 1, 1): (116414, 108424, 131072, 73728),
    (1, 64, 32, 3, 2, 1, 1): (316214, 8414, 32768, 18432),
    (0, 32, 1, 9, 1, 4, 0): (909321, 4214, 41472, 18432),
    (0, 3, 64, 4, 2, 1, 0): (4414, 316114, 16384, 16384),
    (0, 128, 256, 4, 2, 1, 0): (108424, 216424, 524288, 524288),
    (0, 256, 512, 4, 1, 1, 0): (216424, 216424, 2097152, 2097152),
    (0, 512, 1, 4, 1, 1, 0): (909121, 4424, 131072, 65536),
}


def _model_layers():
    from baryon_painter_amd.models import arch as A
    found = []

    def walk(o):
        if isinstance(o, (list, tuple)):
            if len(o) == 2 and isinstance(o[0], str) and isinstance(o[1], dict) and "kernel_size" in o[1]:
                c = o[1]
                found.append((1 if "transp" in o[0] else 0, c["in_channels"], c["out_channels"], c["kernel_size"],
                              c["stride"], c["padding"], c.get("output_padding", 0)))
            else:
                for v in o:
                    walk(v)
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)

    for a in (A.fiducial_architecture(512), A.fiducial_architecture(512, predict_var=True),
              A.cgan_generator_architecture(), A.cgan_discriminator_architecture()):
        walk(a)
    return found


def test_model_layers_keep_their_kernels():
    lib = L.load()
    layers = _model_layers()
    assert len(layers) == 96 and set(layers) == set(MODEL_LAYER_IDS), sorted(set(layers) ^ set(MODEL_LAYER_IDS))
    for conv, want in MODEL_LAYER_IDS.items():
        cv = L.Conv(*conv)
        got = tuple(_ids(lib, conv)) + tuple(lib.bp_conv_bf16_packed_elems(C.byref(cv), d) for d in (L.PACK_FWD, L.PACK_BWD))
        assert got == want, (conv, got, want)
        for d in (L.PACK_FWD, L.PACK_BWD):
            assert lib.bp_conv_bf16_supported(C.byref(cv), d, None, None) == (1 if want[2 + d] > 0 else 0), (conv, d)


# the ids that no layer named in the suite before the sweep reached (ten of them instantiations of the plain kernel)
NEW_IDS = (4211, 4411, 8111, 8214, 8411, 8424, 16114, 16214, 16414, 16424, 108414, 208424, 308214, 416222)
FAMILIES = ("plain-mt4", "plain-mt1", "dma4", "dma8", "dmaf", "wres", "700000", "710000", "720000", "730000", "740000",
            "750000", "760000", "770000", "780001", "780002", "tiny", "small")


def test_dispatcher_coverage_of_the_sweep():
    lib = L.load()
    ids, fam, shapes, cop = (collections.Counter() for _ in range(4))
    per_case_ids, per_case_fam, bf16_ok, pairs = collections.defaultdict(set), collections.defaultdict(set), 0, 0
    for tag, case in S.tagged_cases():
        cv = L.Conv(*case[:7])
        for d in (L.PACK_FWD, L.PACK_BWD):
            kid = lib.bp_conv_kernel_id(C.byref(cv), d)
            pairs += 1
            ids[kid] += 1
            fam[S.family(kid)] += 1
            per_case_ids[kid].add(case)
            per_case_fam[S.family(kid)].add(case)
            assert (lib.bp_conv_packed_floats(C.byref(cv), d) > 0) == (kid >= 0), (tag, case, d, kid)
            ok = lib.bp_conv_bf16_supported(C.byref(cv), d, None, None)
            assert ok in (0, 1) and (lib.bp_conv_bf16_packed_elems(C.byref(cv), d) > 0) == (ok == 1), (tag, case, d)
            bf16_ok += ok
            sh = S.igemm_shape(kid)
            if sh is not None:
                shapes["CC%d" % sh[0]] += 1
                shapes["NT%dxWN%d" % sh[1:]] += 1
                gathered, produced = S.gathered_produced(case, d)
                if S.family(kid).startswith("plain") and case[4] == 1 and produced <= 8 and gathered <= 16:
                    cop["COP%d" % (1 if produced == 1 else 2 if produced == 2 else 4 if produced <= 4 else 8)] += 1
    print("\n%d cases, %d (case, direction) pairs; bp_conv_bf16_supported: %d" % (pairs // 2, pairs, bf16_ok))
    print("family         pairs  cases")
    for f in FAMILIES + ("none",):
        print("  %-12s %5d  %5d" % (f, fam[f], len(per_case_fam[f])))
    print("kernel id      pairs  cases")
    for kid in sorted(ids):
        print("  %-12d %5d  %5d%s" % (kid, ids[kid], len(per_case_ids[kid]), "  (new)" if kid in NEW_IDS else ""))
    print("igemm shapes: " + ", ".join("%s %d" % kv for kv in sorted(shapes.items())))
    print("pixel packing: " + ", ".join("%s %d" % kv for kv in sorted(cop.items())))
    for f in FAMILIES:
        assert len(per_case_fam[f]) >= 3, "family %s is reached by %d cases" % (f, len(per_case_fam[f]))
    for kid in NEW_IDS:
        assert len(per_case_ids[kid]) >= 2, "kernel id %d is reached by %d cases" % (kid, len(per_case_ids[kid]))
    for key in ("CC4", "CC8", "CC16", "NT1xWN1", "NT2xWN1", "NT4xWN1", "NT4xWN2"):
        assert shapes[key] >= 3, key
    for key in ("COP1", "COP2", "COP4", "COP8"):
        assert cop[key] >= 3, key
    assert fam["none"] <= 0.10 * pairs, "more than 10 %% of the pairs have no matrix-core kernel: %d of %d" % (fam["none"], pairs)


# ---------------------------------------------------------------------------------------------------------------------
# The statistics sweep (tests/test_gpu_stats_sweep.py).  bp_conv_stats_workspace and
# bp_conv_backward_data_act_workspace are host arithmetic: the pointers of the views are not dereferenced.
def _layout(c, kind, bf16=False):
    """conv_sweep_gpu._layout, restated (that module needs a device)."""
    if kind == "aligned":
        q = 8 if bf16 else 4
        return (c + q - 1) // q * q + 8, q
    cs = c + 3
    return cs + (cs % 2 == 0), 1


def _fake_view(n, c, h, w, kind, bf16=False):
    cs, co = _layout(c, kind, bf16)
    return L.View(0x100000, n, h, w, c, cs, co, L.BF16 if bf16 else L.F32)


def _stats_ws(lib, case, d, kind, impl, bf16=False):
    """Workspace query for the views test_gpu_stats_sweep.py builds (bf16: every view bf16)."""
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    cv = L.Conv(*case[:7])
    x, y = _fake_view(n, ci, h, w, kind, bf16), _fake_view(n, co, ho, wo, kind, bf16)
    return lib.bp_conv_stats_workspace(C.byref(cv), d, C.byref(x), C.byref(y), impl)


def _act_ws(lib, case, kind, bf16=False):
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    cv = L.Conv(*case[:7])
    dy, g = _fake_view(n, co, ho, wo, kind), _fake_view(n, ci, h, w, kind, bf16)
    return lib.bp_conv_backward_data_act_workspace(C.byref(cv), C.byref(dy), C.byref(g))


# (implementation, layout, direction) -> {family of bp_conv_kernel_id: sweep cases with a non-zero workspace}.  The three
# register-resident forward families of conv_flat.hip (720000, 730000, 740000: 3 cases each) refuse a produced view that is
# not 16-byte addressable; their workspace queries used to answer for it all the same (337 where 328 stands now).  Making
# the queries ask what the kernels ask moved that one row; every other entry is what the commit before computed.
STATS_TABLE = {
    ("mfma", "aligned", 0): {"700000": 4, "720000": 3, "730000": 3, "740000": 3, "760000": 2, "780001": 3, "780002": 3, "dma4": 10,
                             "dma8": 10, "dmaf": 69, "plain-mt1": 16, "plain-mt4": 188, "tiny": 10, "wres": 13},
    ("mfma", "aligned", 1): {"710000": 3, "dma4": 7, "dma8": 10, "dmaf": 46, "plain-mt1": 45, "plain-mt4": 210},
    ("mfma", "odd", 0): {"700000": 4, "760000": 2, "780001": 3, "780002": 3, "dma4": 10, "dma8": 10, "dmaf": 69, "plain-mt1": 16,
                         "plain-mt4": 188, "tiny": 10, "wres": 13},
    # (an odd view drops the weights-resident layers to the plain kernel, which has the mode-2 epilogue: 11 more)
    ("mfma", "odd", 1): {"dma4": 7, "dma8": 10, "dmaf": 46, "plain-mt1": 45, "plain-mt4": 210, "wres": 11},
    ("bf16", "aligned", 0): {"700000": 4, "710000": 2, "720000": 3, "730000": 3, "740000": 3, "750000": 3, "770000": 3, "780001": 3,
                             "780002": 3, "dma4": 5, "dma8": 8, "dmaf": 62, "plain-mt1": 2, "plain-mt4": 94, "small": 18, "tiny": 15,
                             "wres": 17},
    ("bf16", "aligned", 1): {"710000": 3, "720000": 1, "740000": 1, "wres": 2},
    ("bf16", "odd", 0): {},
    ("bf16", "odd", 1): {},
    ("act", "aligned", 1): {"small": 6},
    ("act", "odd", 1): {"small": 6},
    ("act-bf16", "aligned", 1): {"small": 2},
    ("act-bf16", "odd", 1): {},
}


def test_statistics_workspace_table_of_the_sweep():
    lib = L.load()
    got = {key: collections.Counter() for key in STATS_TABLE}
    for tag, case in S.tagged_cases():
        fams = [S.family(i) for i in _ids(lib, case)]
        for kind in ("aligned", "odd"):
            for d in (0, 1):
                if _stats_ws(lib, case, d, kind, L.IMPL_MFMA) > 0:
                    got[("mfma", kind, d)][fams[d]] += 1
                if _stats_ws(lib, case, d, kind, L.IMPL_BF16, True) > 0:
                    got[("bf16", kind, d)][fams[d]] += 1
            if _act_ws(lib, case, kind) > 0:
                got[("act", kind, 1)][fams[1]] += 1
            if _act_ws(lib, case, kind, True) > 0:
                got[("act-bf16", kind, 1)][fams[1]] += 1
    for key, want in STATS_TABLE.items():
        assert dict(got[key]) == want, (key, dict(sorted(got[key].items())))
    assert sum(STATS_TABLE[("mfma", "aligned", 0)].values()) == 337 and sum(STATS_TABLE[("mfma", "aligned", 1)].values()) == 321


def test_fold_plan_and_row_count_from_the_workspace():
    assert [S.fold_plan(r) for r in (1, 2048, 2049, 2064, 8191, 8192, 8208, 70000)] == \
        [(0, 0), (0, 0), (65, 32), (65, 32), (256, 32), (256, 32), (249, 33), (256, 274)]
    for rows in (1, 7, 2048, 2049, 2052, 2064, 8000, 8208, 65535):
        for c in (1, 16, 512):
            assert S.stats_rows((rows + S.fold_plan(rows)[0]) * 16 * c, c) == rows
    assert S.stats_rows((8191 + 256) * 16, 1) is None           # 8191 + 256 = 8198 + 249: not told apart
    assert [S.fold_regime(r) for r in (2048, 2049, 8191, 8192)] == ["direct", "fold32", "fold32", "fold256"]


def test_extra_statistics_cases_sit_in_the_regime_their_tags_name():
    lib = L.load()
    tags = [t for t, _ in S.STATS_EXTRA]
    assert len(set(tags)) == len(tags) and not set(tags) & {t for t, _ in S.tagged_cases()}
    for tag, case in S.STATS_EXTRA:
        assert S.valid(case), tag
        kind, dirn, what = tag.split(":")
        d = 0 if dirn == "f" else 1
        fam = S.family(_ids(lib, case)[d])
        produced = S.gathered_produced(case, d)[1]
        nb = _stats_ws(lib, case, d, "aligned", L.IMPL_MFMA)
        rows = S.stats_rows(nb, produced) if produced & (produced - 1) == 0 else None
        if kind == "rows":
            assert fam in ("plain-mt1", "plain-mt4", "dma4", "dma8", "dmaf"), (tag, fam)
            assert S.fold_regime(rows) == what, (tag, rows)
            assert {"direct": rows == 2048, "fold32": rows % 32 != 0, "fold256": rows % 256 != 0}[what], (tag, rows)
        elif kind == "wres":
            one = _stats_ws(lib, case[:7] + (1,) + case[8:], d, "aligned", L.IMPL_MFMA)
            tiles = case[7] * S.stats_rows(one, produced)
            assert fam == "wres" and rows < tiles and tiles > 512, (tag, fam, rows, tiles)     # workgroups < tiles
        elif kind == "wide":
            assert produced == int(what) and (nb > 0) == (produced <= 512), (tag, nb)
            assert nb == 0 or rows <= 4, (tag, rows)
        elif what == "act":
            nb = _act_ws(lib, case, "aligned")
            assert fam == "small" and S.fold_regime(S.stats_rows(nb, None, 32)) == "fold32", (tag, nb)     # rows of 3 x 8 -> 32 doubles
        else:
            want = {"stem": "700000", "flat_t4": "720000", "flat_g4": "730000", "flat_t64": "740000", "enc": "760000",
                    "enc0": "780002", "tiny": "tiny"}[what]
            assert fam == want, (tag, fam)
            # workgroups = the family's cap, below the number of tiles (a grid-stride walk); the one-channel kernel: a fold
            cap = {"stem": 2048, "flat_t4": 512, "flat_g4": 256, "flat_t64": 256, "enc": 512, "enc0": 2048}.get(what)
            if cap is None:
                assert S.fold_regime(rows) == "fold32", (tag, rows)
            else:
                one = S.stats_rows(_stats_ws(lib, case[:7] + (1,) + case[8:], d, "aligned", L.IMPL_MFMA), produced)
                assert rows == cap and case[7] * one > cap, (tag, rows, one)
    # every power of two up to 512 produced channels has the epilogue, 1024 has not: stats_plan's LDS condition refuses none
    for c in (16, 32, 64, 128, 256, 512, 1024):
        for conv in ((0, 4, c, 1, 1, 0, 0), (0, 16, c, 3, 1, 1, 0), (1, 8, c, 4, 2, 1, 0)):
            assert (_stats_ws(lib, conv + (1, 5, 20), 0, "aligned", L.IMPL_MFMA) > 0) == (c <= 512), (c, conv)


def test_counting_operands_give_integers_and_stay_below_2_24():
    """counting_reference is the float64 convolution of counting_inputs; every term of every sum is on its grid; the share
    of (case, direction) pairs with a workspace whose Q reaches 2^24 -- what the GPU file skips -- is at most 5 %."""
    lib = L.load()
    over = total = 0
    cases = S.stats_cases()
    assert len(cases) == PINNED_LEN + len(S.STATS_EXTRA) + len(S.STATS_REGRESSIONS) and all(S.valid(c) for _, c in cases)
    assert len({t for t, _ in cases}) == len(cases)
    for i, (tag, case) in enumerate(cases):
        T = S.terms(case)
        cy, cdx = S.counting_reference(case, 0, T), S.counting_reference(case, 1, T)
        x, wf = S.counting_inputs(case, i, 0)
        dy, wb, raw, pw = S.counting_inputs(case, i, 1)
        assert set(np.unique(raw)) <= {1.0, 2.0} and cy.shape[1] == case[2] and cdx.shape == raw.shape
        if i % 29 == 0 or (i >= PINNED_LEN and S._macs(case) < 4e7):
            y = S._conv4(case, x.astype(np.float64), wf.astype(np.float64), None, dy.astype(np.float64))[0]
            dx = S._conv4(case, x.astype(np.float64), wb.astype(np.float64), None, dy.astype(np.float64))[1]
            assert np.array_equal(y, cy) and np.array_equal(dx, cdx), tag
        if case[1] > 1:
            assert not np.array_equal(raw[0, 0], raw[0, 1]), "the pattern differs per channel"
        assert (cy == np.round(cy)).all() and (cdx == np.round(cdx)).all() and cy.max() <= case[3] ** 2
        sums, mags, g = S.stats_reference(3, cdx, raw, pw)
        for v in sums + mags:
            assert (4 * v == np.round(4 * v)).all(), tag
        assert (S.bf16_round(g.astype(np.float32)) == g).all() and (S.bf16_round(cy.astype(np.float32)) == cy).all()
        q = [(cy * cy).sum(axis=(0, 2, 3)).max(), 4 * max(mags[1].max(), mags[2].max())]
        for d in (0, 1):
            if _stats_ws(lib, case, d, "aligned", L.IMPL_MFMA) > 0:
                total += 1
                over += q[d] >= 2.0 ** 24
                assert i < PINNED_LEN or q[d] < 2.0 ** 24, "an extra case must stay exact: %s" % tag
    print("\n%d of %d (case, direction) pairs with a workspace reach Q = 2^24" % (over, total))
    assert over <= 0.05 * total


def test_stats_reference_against_a_direct_restatement():
    rng = np.random.Generator(np.random.PCG64(5))
    for shape in ((2, 3, 5, 7), (1, 8, 4, 4), (3, 1, 9, 2)):
        n, c, h, w = shape
        dx = rng.standard_normal(shape).astype(np.float32)
        raw = rng.standard_normal(shape).astype(np.float32)
        scale, shift = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.4, 0.4, c).astype(np.float32)
        slope = rng.uniform(0.05, 0.3, c).astype(np.float32)
        slope[::3] = 0.0
        want = np.zeros((5, c))
        mag = np.zeros((5, c))
        for ch in range(c):
            for i in range(n):
                for yy in range(h):
                    for xx in range(w):
                        d, r = dx[i, ch, yy, xx], raw[i, ch, yy, xx]
                        t = np.float32(np.float64(r) * np.float64(scale[ch]) + np.float64(shift[ch]))
                        g = np.float64(d) if t > 0 else np.float64(np.float32(d * slope[ch]))
                        terms = (np.float64(d), np.float64(d) ** 2, g, g * np.float64(r), 0.0 if t > 0 else np.float64(d) * np.float64(t))
                        want[:, ch] += terms
                        mag[:, ch] += np.abs(terms)
        s1, m1, _ = S.stats_reference(1, dx.astype(np.float64))
        s3, m3, g3 = S.stats_reference(3, dx.astype(np.float64), raw, (scale, shift, slope))
        s2, m2, _ = S.stats_reference(2, dx.astype(np.float64), raw, (scale, shift, slope))
        assert len(s2) == 2 and len(s3) == 3 and g3.shape == shape
        for got, ref in zip(s1 + s3 + m1 + m3, list(want) + list(mag)):
            assert np.allclose(got, ref, rtol=1e-13, atol=1e-13)
        assert np.array_equal(s2[0], s3[0]) and np.array_equal(s2[1], s3[1]) and np.array_equal(m2[1], m3[1])
