"""CPU: the cases of tests/wgrad_sweep.py sit where they claim to, by bp_conv_backward_weight_plan.

The weight-gradient sweep reaches the second and third iteration of every tile loop by extent alone; whether a case
does is host arithmetic -- the kernel the dispatcher picks, its cap and its tile -- and is checked here without a GPU:
the plan names the family each case is listed under, its nsplit is min(units, cap) of the module's table, the case is in
its regime, its integer data stay in the exact range, and the plan never needs more than the workspace query grants.
tests/golden/wgrad_plan.json records every plan row; a retuned heuristic shows here first and the case is re-picked.
tests/golden/wgrad_dispatch.json records the same queries over the conv sweep and the models' layers, under every
environment switch that moves a layer between the weight-gradient families.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from baryon_painter_amd import _lib as L

import conv_sweep as S
import wgrad_sweep as W
from golden import make_wgrad_dispatch as MD
from golden import make_wgrad_plan as M

QUERY = {q[0]: i for i, q in enumerate(M.QUERIES)}
PART = {"stem": 1280, "flat": 7168, "flat_s2": 8192}          # floats of one partial row of the self-reducing kernels


@pytest.fixture(scope="module")
def rows():
    return M.compute()


def _family(row):
    return L.WGRAD_FAMILIES[row[1]] if row[1] >= 0 else None


def test_plan_rows_equal_the_recorded_table(rows):
    doc = M.load()
    assert doc["queries"] == [q[0] for q in M.QUERIES]
    assert doc["tags"] == [e.tag for e in W.ENTRIES] and doc["cases"] == [list(e.case) for e in W.ENTRIES]
    wrong = ["%s %s: got %s, recorded %s" % (e.tag, q[0], g, w)
             for e, got, want in zip(W.ENTRIES, rows, doc["rows"]) for q, g, w in zip(M.QUERIES, got, want) if g != w]
    assert not wrong, "%d rows differ:\n%s" % (len(wrong), "\n".join(wrong[:40]))


def test_every_case_is_served_by_the_family_and_split_count_it_is_listed_under(rows):
    wrong = []
    for e, r in zip(W.ENTRIES, rows):
        if e.impl == "bf16":
            queries = [("bf16:aligned:" + e.dt, e.inst, False)]
        else:
            queries = [("%s:%s:ff" % (impl, kind), W.expected_inst(e, kind), impl == "shared")
                       for kind in ("aligned", "odd") for impl in ("mfma", "shared", "auto")]
        for q, inst, shared in queries:
            rc, fam, ns = r[QUERY[q]][0], _family(r[QUERY[q]]), r[QUERY[q]][2]
            want = (L.BP_OK, W.INST[inst].family, W.nsplit(inst, e.case, shared))
            if (rc, fam, ns) != want:
                wrong.append("%s %s: plan (rc, family, nsplit) = %s, the table says %s (%s)" % (W.case_id(e), q, (rc, fam, ns), want, inst))
    assert not wrong, "\n".join(wrong[:40])


def test_every_case_sits_in_its_regime():
    for e in W.ENTRIES:
        assert e.case[7] >= 2 and W.in_regime(e.inst, e.case, e.regime), W.case_id(e)
        r = W.INST[e.inst]
        if r.tw:
            n, yh, yw = W.y_extent(e.case)
            assert yh % r.th and yw % r.tw, "%s: extents are multiples of the tile" % W.case_id(e)
        assert W.tensor_bytes(e.case) <= W.MAX_TENSOR_BYTES, W.case_id(e)
    # every promised (family, regime) is there; a regime B left out is listed, and does not fit
    for inst, kind, conv, regimes, impl, dt in W.LAYERS:
        for regime in regimes:
            present = any(e.inst == inst and e.regime == regime and e.case[:7] == conv for e in W.ENTRIES)
            assert present != (regime == "B" and (inst, conv) in W.DROPPED_B), (inst, conv, regime)
    for (inst, conv), why in W.DROPPED_B.items():
        case = W.pick(inst, conv, "B")
        (ho, wo), n, co = S.out_shape(case), case[7], case[2]
        dy = (W.draws(n * ho * wo * co, 2, 3) - 1).to(torch.float32).reshape(n, ho, wo, co)
        too_big = W.tensor_bytes(case) > W.MAX_TENSOR_BYTES
        too_many = W.magnitude_bound(dy, W.int_pointwise(case, 0)) >= W.EXACT_LIMIT
        assert too_big or too_many, "%s %s fits: %s" % (inst, conv, why)


def test_the_shared_plan_differs_for_a_tap_blocked_case(rows):
    n = sum(1 for e, r in zip(W.ENTRIES, rows) if W.INST[e.inst].family in ("tiles", "tiles_dma") and
            r[QUERY["mfma:%s:ff" % e.kind]][2] != r[QUERY["shared:%s:ff" % e.kind]][2])
    assert n > 0


def test_the_existing_sweep_never_reaches_a_second_tile():
    """At the extents of tests/conv_sweep.py every split has exactly one tile: nsplit is the number of tiles of one of
    the family's tile shapes (the gap the weight-gradient sweep closes)."""
    lib = L.load()
    shapes = {}
    for r in W.INST.values():
        shapes.setdefault(r.family, set()).add((r.tw, r.th))
    seen = set()
    for tag, case in S.tagged_cases():
        n, yh, yw = W.y_extent(case)
        for kind in ("aligned", "odd"):
            rc, fam, ns, cxp, cyp, ws = M.plan(lib, L, case, "mfma", kind, "ff")
            if rc != L.BP_OK:
                continue
            fam = L.WGRAD_FAMILIES[fam]
            seen.add(fam)
            if fam == "thin_c1":
                assert ns == -(-(n * -(-yh // 16) * -(-yw // 4)) // 256), (tag, ns)
            elif fam in ("ws_f32", "direct"):
                continue
            else:
                tiles = {n * -(-yw // tw) * -(-yh // th) for tw, th in shapes[fam]}
                assert ns in tiles, "%s [%s]: %s has nsplit %d, tiles %s" % (tag, kind, fam, ns, sorted(tiles))
    assert {"tiles", "tiles_dma", "small", "general", "enc", "thin_cy1", "stem", "flat", "flat_s2", "small_chunked"} <= seen


def test_integer_data_stay_in_the_exact_range():
    for i, e in enumerate(W.ENTRIES):
        tr, ci, co, k, s, p, op, n, h, w = e.case
        ho, wo = S.out_shape(e.case)
        dy = (W.draws(n * ho * wo * co, 2 * i + 2, 3) - 1).to(torch.float32).reshape(n, ho, wo, co)
        assert W.magnitude_bound(dy, W.int_pointwise(e.case, i)) < W.EXACT_LIMIT, W.case_id(e)
    # the draws cover their ranges evenly, and the activation makes multiples of 1/4 no larger than max_activation
    x, dy, pw = W.int_inputs((0, 6, 5, 3, 1, 1, 0, 2, 37, 41), 3)
    assert sorted(x.unique().tolist()) == [-2, -1, 0, 1, 2] and sorted(dy.unique().tolist()) == [-1, 0, 1]
    assert abs(float(x.mean())) < 0.05 and abs(float(dy.mean())) < 0.05
    xa = W.activated(x, pw)
    assert bool((xa * 4 == (xa * 4).round()).all()) and float(xa.abs().max()) <= W.max_activation(pw)
    assert bool((xa.to(torch.bfloat16).double() == xa).all())
    assert bool((W.activated(torch.zeros(1, 1, 1, 6), pw) != 0).all())


def test_plan_bytes_never_exceed_the_workspace_query(rows):
    for e, r in zip(W.ENTRIES, rows):
        k = e.case[3]
        for q, (rc, fam, ns, cxp, cyp, ws) in zip(M.QUERIES, r):
            if rc != L.BP_OK:
                assert fam == -1 and ns == 0
                continue
            name = L.WGRAD_FAMILIES[fam]
            need = ns * PART[name] * 4 + -(-ns // 32) * PART[name] * 8 if name in PART else ns * k * k * cxp * cyp * 4
            assert 0 < ws and need <= ws, (W.case_id(e), q[0], name, need, ws)
            assert (ns == 0) == (name == "direct")


def test_dispatch_rows_equal_the_recorded_table_under_every_switch():
    """tests/golden/wgrad_dispatch.json: the same queries over the conv sweep and the models' layers, under the default
    setting and under every environment switch that moves a weight-gradient layer between families."""
    doc = MD.load()
    tagged = MD.cases()
    assert doc["queries"] == [q[0] for q in MD.QUERIES] and len(doc["default"]) == len(tagged)
    assert MD.D.load()["tags"] == [t for t, _ in tagged]          # (the cases are dispatch_table.json's)
    assert set(doc["settings"]) == set(MD.SWITCHES)
    want = MD.unpack(doc)
    # (the switches are read once into statics: one child process per setting, all at once)
    with ThreadPoolExecutor(max_workers=len(MD.SETTINGS)) as ex:
        got = dict(zip(MD.SETTINGS, ex.map(MD.compute_setting, MD.SETTINGS)))
    wrong = []
    for s in MD.SETTINGS:
        assert len(got[s]) == len(want[s]) == len(tagged)
        for (tag, case), g, w in zip(tagged, got[s], want[s]):
            wrong += ["%s %s %s [%s]: got %s, recorded %s" % (tag, case, q[0], s or "default", a, b)
                      for q, a, b in zip(MD.QUERIES, g, w) if a != b]
            # the plan never needs more than the workspace query grants
            k = case[3]
            for q, (rc, fam, ns, cxp, cyp, ws) in zip(MD.QUERIES, g):
                if rc != L.BP_OK:
                    assert fam == -1 and ns == 0, (tag, q[0], s)
                    continue
                name = L.WGRAD_FAMILIES[fam]
                need = ns * PART[name] * 4 + -(-ns // 32) * PART[name] * 8 if name in PART else ns * k * k * cxp * cyp * 4
                assert 0 < ws and need <= ws, (tag, q[0], s, name, need, ws)
    print("\n%d settings x %d cases x %d queries compared" % (len(MD.SETTINGS), len(tagged), len(MD.QUERIES)))
    assert not wrong, "%d rows differ:\n%s" % (len(wrong), "\n".join(wrong[:40]))
    # the default setting reaches every family: the table cannot silently lose one
    for table in (got, want):
        reached = {L.WGRAD_FAMILIES[r[1]] for rows_ in table[""] for r in rows_ if r[0] == L.BP_OK}
        assert reached == set(L.WGRAD_FAMILIES) and len(reached) == 18, sorted(set(L.WGRAD_FAMILIES) - reached)


@pytest.mark.parametrize("case", [(0, 5, 7, 3, 1, 1, 0, 2, 9, 11), (0, 3, 4, 4, 2, 0, 0, 2, 11, 13), (1, 4, 3, 5, 3, 2, 1, 2, 5, 6)],
                         ids=["conv_k3", "conv_k4s2_trailing", "transposed_k5s3_outpad"])
def test_reference_agrees_with_the_sweeps(case):
    x, w, bias, dy, pw = S.make_inputs(case, 5, False)
    want = S.reference(case, x, w, None, dy, pw)[2]
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    dyt = torch.from_numpy(np.ascontiguousarray(dy.transpose(0, 2, 3, 1)))
    got = W.reference_dw(case, W.activated(xt, tuple(torch.from_numpy(v) for v in pw)), dyt.double()).numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert (W.terms_dw(case).numpy()[0, 0] == S.terms(case)[2][0, 0]).all()
    # ... and the bf16 staging
    want_b = S.reference(case, x, w, None, S.bf16_round(dy), pw, S.bf16_round)[2]
    got_b = W.reference_dw(case, W.activated(xt, tuple(torch.from_numpy(v) for v in pw), True), dyt.to(torch.bfloat16).double()).numpy()
    assert np.abs(got_b - want_b).max() <= 1e-12 * np.abs(want_b).max()
