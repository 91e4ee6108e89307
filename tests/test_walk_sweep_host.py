"""CPU: the cases of tests/walk_sweep.py walk where they claim to, by the library's own host answers.

Whether a workgroup of a persistent kernel walks three tiles is host arithmetic -- the kernel the dispatcher picks, its
tile and its cap -- and is checked here without a GPU: bp_conv_kernel_id names the family each case is listed under, the
restated launch gives every workgroup at least three tiles, some four, with a ragged remainder, at the smallest such
batch; where the family has a statistics epilogue the restated grid is the row count behind bp_conv_stats_workspace,
which is the library's own grid (for the bf16 kernels, whose rows are per tile: the library's own tile count); and the
operands of the exact pass keep every partial sum in the range fp32 adds exactly.

The caps are read from the environment once per process: with any of them set the restated arithmetic would describe
another launch than the one that runs, so the module raises.
"""
import ctypes as C

import numpy as np
import pytest

from baryon_painter_amd import _lib as L

import conv_sweep as S
import walk_sweep as W
from conv_sweep_gpu import _layout

W.require_production_environment()

# cases whose family writes one row of partial sums per workgroup in the listed direction (mode 1 forward, mode 2 data
# gradient): pinned, so that a check that silently stopped applying shows
STATS_TAGS = {"stem:f", "flat_k7:d", "flat_t4:f", "flat_t64:f", "flat_g4:f", "enc_fwd:f", "enc0_1:f", "enc0_2:f", "wres:f"}
# ... and the bf16 forward cases, whose rows are one per (phase, tile)
BF16_STATS_TAGS = {"bf16_p:16_32:f", "bf16_pf:T32_16:f", "bf16_p:T16_8:f", "bf16_p:1_8:f", "bf16_p:2_8:f"}


def _view(shape, kind="aligned", bf16=False):
    n, c, h, w = shape
    cs, co = _layout(c, kind, bf16)
    return L.View(0x10000, n, h, w, c, cs, co, L.BF16 if bf16 else L.F32)


def _module_views(e, bf16=False):
    gs, ps = W.operand_shapes(e.case, e.direction)
    gv, pv = _view(gs, bf16=bf16), _view(ps, bf16=bf16)
    return (gv, pv) if e.direction == W.FWD else (pv, gv)


IDS = [W.case_id(e) for e in W.ENTRIES]


def test_tags_are_unique_and_every_record_is_used():
    assert len(set(IDS)) == len(IDS)
    assert {e.inst for e in W.ENTRIES} == set(W.INST)
    assert all(e.impl in ("mfma", "bf16") and (e.impl == "bf16") == (W.INST[e.inst].kid is None) for e in W.ENTRIES)


@pytest.mark.parametrize("e", W.ENTRIES, ids=IDS)
def test_the_dispatcher_serves_the_case_with_the_listed_kernel(e):
    lib = L.load()
    cv = L.Conv(*e.case[:7])
    assert S.valid(e.case)
    if e.impl == "mfma":
        assert lib.bp_conv_kernel_id(C.byref(cv), e.direction) == W.INST[e.inst].kid
        return
    # the bf16 kernels have no id: the restated b_config names the persistent form, and the library takes these views
    assert W.bf16_inst(e.case, e.direction) == e.inst
    gs, ps = W.operand_shapes(e.case, e.direction)
    for ib, ob in ((True, True), (False, False), (False, True), (True, False)):
        gv, pv = _view(gs, bf16=ib), _view(ps, bf16=ob)
        assert lib.bp_conv_bf16_supported(C.byref(cv), e.direction, C.byref(gv), C.byref(pv)) == 1, (ib, ob)


def test_every_persistent_bf16_form_of_the_layers_is_listed():
    listed = {(e.case[:7], e.direction) for e in W.ENTRIES if e.impl == "bf16"}
    found = {(conv, d) for conv in W.LAYERS for d in (W.FWD, W.BWD) if W.bf16_inst(conv + (1, 40, 40), d)}
    assert found == listed


@pytest.mark.parametrize("e", W.ENTRIES, ids=IDS)
def test_every_workgroup_walks_three_tiles_and_some_four(e):
    r = W.INST[e.inst]
    ty, tx = W.tiles(e)
    assert (ty, tx) == (3, 3)
    _, (n, c, h, w) = W.operand_shapes(e.case, e.direction)
    phase = W.geom(e.case, e.direction)["OS"]
    assert r.kid is None or r.phase == phase
    assert (-(-h // phase), -(-w // phase)) == (2 * r.th + 1, 2 * r.tw + 1)
    nt, grid, lo, hi = W.plan(e)
    assert nt == 9 * e.case[7] and lo >= 3 and hi >= 4 and hi > lo
    if r.walk == "stride":
        assert grid == r.cap and nt > 3 * r.cap and nt % r.cap != 0
    else:
        assert nt == (grid - 1) * hi + lo                            # runs of `hi` tiles and a shorter last one
    # the walks themselves: tile t is tile t % 9 of image t // 9; the tiles of row 2 and column 2 are clipped
    walks = W.walks(e)
    assert sorted(t for wk in walks for t in wk) == list(range(nt))
    assert min(map(len, walks)) == lo and max(map(len, walks)) == hi
    clipped = lambda t: t % 9 // 3 == 2 or t % 3 == 2
    stale = sum(1 for wk in walks if any(clipped(a) and not clipped(b) for a, b in zip(wk, wk[1:])))
    crossing = sum(1 for wk in walks if wk[0] // 9 != wk[-1] // 9)
    kinds = min(len({t % 9 for t in wk}) for wk in walks)
    # (a full tile after a clipped one: 5 of the 9 tiles are clipped, a walk has two or three steps -- a quarter at least)
    if r.walk == "stride":         # every walk crosses images and meets three kinds of tile
        assert crossing == grid and kinds >= 3 and 4 * stale > grid
    else:                          # (a run of four of the nine tiles of an image: some runs cross, all see two kinds)
        assert crossing >= grid // 4 and kinds >= 2 and 4 * stale > grid
    assert e.case[7] == W.smallest_n(e), "n = %d is not the smallest batch with such a walk (%d)" % (e.case[7], W.smallest_n(e))


@pytest.mark.parametrize("e", W.ENTRIES, ids=IDS)
def test_the_restated_grid_is_the_librarys_own(e):
    lib = L.load()
    cv = L.Conv(*e.case[:7])
    _, (n, pc, h, w) = W.operand_shapes(e.case, e.direction)
    nt, grid, lo, hi = W.plan(e)
    if e.impl == "mfma":
        x, y = _module_views(e)
        nbytes = lib.bp_conv_stats_workspace(C.byref(cv), e.direction, C.byref(x), C.byref(y), L.IMPL_MFMA)
        assert (nbytes > 0) == (e.tag in STATS_TAGS)
        if nbytes:
            assert S.stats_rows(nbytes, pc) == grid
        return
    x, y = _module_views(e)                                          # (fp32 views: no other bf16 kernel takes those)
    nbytes = lib.bp_conv_stats_workspace(C.byref(cv), e.direction, C.byref(x), C.byref(y), L.IMPL_BF16)
    assert (nbytes > 0) == (e.tag in BF16_STATS_TAGS)
    if nbytes:
        assert S.stats_rows(nbytes, pc) == W.geom(e.case, e.direction)["nphase"] ** 2 * nt


def test_exact_operands_stay_in_the_exact_range():
    for i, e in enumerate(W.ENTRIES):
        assert W.exact_magnitude(e) < W.EXACT_LIMIT, W.case_id(e)
    # the draws cover their ranges, the activation makes half-integers no larger than the bound assumes, act(0) != 0 on
    # the first channel, and every operand is exact in bf16
    e = W.Entry("probe", "flat_k7", W.FWD, "mfma", (0, 8, 16, 7, 1, 3, 0, 2, 9, 11))
    g, w, bias, pw = W.exact_inputs(e, 0)
    assert sorted(np.unique(g)) == [-2, -1, 0, 1, 2] and sorted(np.unique(w)) == [-1, 0, 1]
    assert bias is not None and np.abs(bias).max() <= W.MAX_BIAS and W.exact_inputs(e, 1)[2] is None
    a = S.activated(g, pw)
    assert (a * 2 == np.round(a * 2)).all() and np.abs(a).max() <= W.MAX_X + 1
    assert (S.bf16_round(a.astype(np.float32)) == a).all()
    assert S.activated(np.zeros((1, 8, 1, 1), np.float32), pw)[0, 0, 0, 0] != 0
    assert set(np.unique(pw[2])) <= {0.0, 0.5, 1.0} and set(np.unique(pw[1])) <= {0.0, 1.0} and (pw[0] == 1).all()
    gd, wd, bd, pwd = W.exact_inputs(e._replace(direction=W.BWD), 0)
    assert bd is None and pwd is None and gd.shape == (2, 16, 9, 11)


@pytest.mark.parametrize("case", [(0, 5, 7, 3, 1, 1, 0, 2, 9, 11), (0, 3, 4, 4, 2, 0, 0, 2, 11, 13), (1, 4, 3, 5, 3, 2, 1, 2, 5, 6),
                                  (0, 3, 5, 8, 4, 2, 0, 2, 17, 22), (1, 6, 4, 4, 2, 1, 0, 2, 5, 7)],
                         ids=["conv_k3", "conv_k4s2_trailing", "transposed_k5s3_outpad", "conv_k8s4_trailing", "transposed_k4s2"])
def test_reference_agrees_with_the_sweeps(case):
    x, w, bias, dy, pw = S.make_inputs(case, 5, True)
    y, dx = S.reference(case, x, w, bias, dy, pw)[:2]
    yb, dxb = S.bound(case, x, w, bias, dy, pw)[:2]
    Ty, Tdx = S.terms(case)[:2]
    for d, g, b, p, want, want_b, T in ((W.FWD, x, bias, pw, y, yb, Ty), (W.BWD, dy, None, None, dx, dxb, Tdx)):
        got = W.reference(case, d, g, w, b, p)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(W.bound(case, d, g, w, b, p) - want_b).max() <= 1e-12 * np.abs(want_b).max()
        assert (np.broadcast_to(W.terms(case, d), T.shape) == T).all()
    # ... and the bf16 staging
    want = S.reference(case, x, S.bf16_round(w), None, S.bf16_round(dy), pw, S.bf16_round)
    got = W.reference(case, W.FWD, x, S.bf16_round(w), None, pw, S.bf16_round)
    assert np.abs(got - want[0]).max() <= 1e-12 * np.abs(want[0]).max()
    got = W.reference(case, W.BWD, S.bf16_round(dy), S.bf16_round(w), None, None, S.bf16_round)
    assert np.abs(got - want[1]).max() <= 1e-12 * np.abs(want[1]).max()
