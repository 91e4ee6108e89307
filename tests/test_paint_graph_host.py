"""CPU: the parameter block of a paint slot (models/paint_graph.py ParamBlock) -- byte offsets against the values the
models' and the painter's own loops gave before the block had one owner, and the host views the painter fills."""
import numpy as np
import pytest
import torch

from baryon_painter_amd.models.paint_graph import ParamBlock, paint_fields, paint_levels
from baryon_painter_amd.painter import _fill_block, _seed_word

# n = 3: the float32 ``aux`` field is 12 bytes and rounds up to 16; ``tile_ids`` is 24 bytes, ``seed`` 8.
CASES = {
    "cvae shift-log": ((3, 2, 1), {"xf_in": 0, "xf_out": 48, "tile_ids": 96, "seed": 120, "aux": 128}, 144),
    "cvae modes": ((3, 4, 1), {"xf_in": 0, "xf_out": 96, "tile_ids": 192, "seed": 216, "aux": 224}, 240),
    "cgan": ((3, 3, 1), {"xf_in": 0, "xf_out": 72, "tile_ids": 144, "seed": 168, "aux": 176}, 192),
}


@pytest.mark.parametrize("case", list(CASES))
def test_layout_is_the_one_the_models_wrote_out(case):
    (n, xw, aw), offsets, nbytes = CASES[case]
    block = ParamBlock(paint_fields(n, xw, aw))
    assert list(block.layout) == ["xf_in", "xf_out", "tile_ids", "seed", "aux"]
    assert {k: v[0] for k, v in block.layout.items()} == offsets
    assert block.nbytes == nbytes
    assert block.layout["xf_in"] == (0, torch.float64, (n, xw)) and block.layout["xf_out"][1:] == (torch.float64, (n, xw))
    assert block.layout["tile_ids"][1:] == (torch.int64, (n,)) and block.layout["seed"][1:] == (torch.int64, (1,))
    assert block.layout["aux"][1:] == (torch.float32, (n, aw))


def test_fields_are_taken_in_order_and_rounded_up_to_eight_bytes():
    block = ParamBlock([("a", torch.float32, (3,)), ("b", torch.uint8, (1,)), ("c", torch.float64, (2, 2))])
    assert block.layout == {"a": (0, torch.float32, (3,)), "b": (16, torch.uint8, (1,)), "c": (24, torch.float64, (2, 2))}
    assert block.nbytes == 56
    with pytest.raises(ValueError):
        block.views(torch.zeros(55, dtype=torch.uint8))
    with pytest.raises(ValueError):
        block.views(torch.zeros(14, dtype=torch.float32))


@pytest.mark.parametrize("case", list(CASES))
def test_host_views_alias_the_buffer_and_a_short_batch_repeats_its_last_tile(case):
    (n, xw, aw), offsets, nbytes = CASES[case]
    block = ParamBlock(paint_fields(n, xw, aw))
    buf = torch.zeros(block.nbytes, dtype=torch.uint8)
    hv = block.views(buf)
    assert all(isinstance(v, np.ndarray) for v in hv.values())
    assert {k: (v.dtype, v.shape) for k, v in hv.items()} == {
        "xf_in": (np.float64, (n, xw)), "xf_out": (np.float64, (n, xw)), "tile_ids": (np.int64, (n,)),
        "seed": (np.int64, (1,)), "aux": (np.float32, (n, aw))}
    params = {"xf_in": np.arange(2 * xw, dtype=np.float64).reshape(2, xw) + 0.5,
              "xf_out": -np.arange(2 * xw, dtype=np.float64).reshape(2, xw) - 0.25,
              "aux": np.array([0.125, 2.5])}
    ids = np.array([1000, 2 ** 40 + 7], dtype=np.int64)
    hv["seed"][0] = _seed_word(2 ** 64 - 3)
    _fill_block(hv, params, ids, 0, 2, n)                 # 2 tiles into 3 rows
    assert np.array_equal(hv["xf_in"][:2], params["xf_in"]) and np.array_equal(hv["xf_out"][:2], params["xf_out"])
    assert np.array_equal(hv["aux"][:2, 0], params["aux"].astype(np.float32)) and np.array_equal(hv["tile_ids"][:2], ids)
    for k in ("xf_in", "xf_out", "aux", "tile_ids"):
        assert np.array_equal(hv[k][2], hv[k][1]), k
    # the same bytes through a second set of views, and at the stated offsets
    again = block.views(buf)
    for k in hv:
        assert np.array_equal(again[k], hv[k]), k
    assert again["seed"][0] == -3
    raw = buf.numpy()
    assert np.array_equal(raw[offsets["xf_out"]:offsets["xf_out"] + 8].view(np.float64), [-0.25])
    assert np.array_equal(raw[offsets["tile_ids"] + 8:offsets["tile_ids"] + 24].view(np.int64), [2 ** 40 + 7] * 2)
    assert np.array_equal(raw[offsets["aux"]:offsets["aux"] + 12].view(np.float32), np.float32([0.125, 2.5, 2.5]))
    assert not raw[offsets["aux"] + 12:].any()            # the padding of the last field stays untouched


# ------------------------------------------------------------------------------------------- the geometry rule
def _scales(levels):
    return None if levels == 1 else {"n_scale": levels - 1, "step_size": 2.0, "include_original": True}


@pytest.mark.parametrize("ensemble", [False, True])
@pytest.mark.parametrize("p_y_in", [False, True])
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("F", [1, 2])
def test_geometry_rule_of_the_captured_pipeline(F, levels, p_y_in, ensemble):
    """dim_y[0] = levels, dim_x[0] = F levels; no split-scale with a p_y_in network; L = 1 unless an ensemble.  Per
    point of the table the good case, and each axis gone wrong on its own."""
    sc = _scales(levels)
    split_with_net = sc is not None and p_y_in

    def rule(cy=levels, cx=F * levels, L=1, **kw):
        return paint_levels(cy, cx, p_y_in, L, sc, F, ensemble, **kw)
    if split_with_net:
        for L in (1, 2):
            with pytest.raises(NotImplementedError, match="p_y_in"):
                rule(L=L)
    else:
        assert rule() == levels
        if ensemble:
            assert rule(L=2) == levels
        else:
            with pytest.raises(NotImplementedError, match="captured.*L = 1"):
                rule(L=2)
    # the channels are looked at first, and the caller names the exception (the painter: NotImplementedError)
    for bad in ({"cy": levels + 1}, {"cx": F * levels + 1}, {"cx": levels} if F > 1 else {"cx": 2 * levels}):
        with pytest.raises(ValueError, match="dim_y") as e:
            rule(**bad)
        assert not isinstance(e.value, NotImplementedError)
        with pytest.raises(NotImplementedError, match="captured"):
            rule(mismatch=NotImplementedError, **bad)


def test_geometry_rule_counts_the_original_as_a_level():
    assert paint_levels(2, 2, False, 1, {"n_scale": 2, "step_size": 2.0, "include_original": False}, 1, False) == 2
    assert paint_levels(3, 6, False, 1, {"n_scale": 2, "step_size": 2.0, "include_original": True}, 2, False) == 3
    with pytest.raises(ValueError):
        paint_levels(3, 3, False, 1, {"n_scale": 2, "step_size": 2.0, "include_original": False}, 1, False)
