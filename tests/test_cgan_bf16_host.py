"""CPU: what the CGAN's bf16 paint policy rests on and that needs no GPU -- which widths the weights-stationary bf16 k3
kernel takes (host arithmetic of bp_conv_ws_kind: the view pointers are never dereferenced), the dtype of every layer's
views under the policy against bp_conv_bf16_supported, and the ``paint_dtype`` key of a checkpoint's metadata."""
import collections
import ctypes as C

import pytest
import torch

from baryon_painter_amd import _lib as L
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.models.cgan import _GanPaintPlan
from baryon_painter_amd.painter import CGANPainter

BATCHES = (1, 3, 4, 11, 64)


def _kinds(lib, w, h, cstride=128 + 8, coff=8):
    """bp_conv_ws_kind of Conv(0, 128, 128, 3, 1, 1) on bf16 views, both pack directions, every batch size."""
    cv = L.Conv(0, 128, 128, 3, 1, 1, 0)
    out = set()
    for d in (L.PACK_FWD, L.PACK_BWD):
        for n in BATCHES:
            vin = L.View(0x10000, n, h, w, 128, cstride, coff, L.BF16)
            vout = L.View(0x4000000, n, h, w, 128, cstride, coff, L.BF16)
            out.add(lib.bp_conv_ws_kind(C.byref(cv), d, C.byref(vin), C.byref(vout)))
    return out


@pytest.mark.parametrize("h", [8, 128])
def test_stationary_kernel_takes_the_strip_widths_at_every_batch_size(h):
    lib = L.load()
    for w in (16, 32, 64, 128, 192):
        assert _kinds(lib, w, h) == {3}, w
        assert _kinds(lib, w, h, cstride=128, coff=0) == {3}, w
    for w in (48, 96, 160):
        assert _kinds(lib, w, h) == {0}, w
    # strips end at 256 pixels (four strips); wider layers stay on the tiled kernel
    assert _kinds(lib, 256, h) == {3} and _kinds(lib, 320, h) == {0} and _kinds(lib, 512, h) == {0}
    # (a channel stride that is no multiple of 8 elements has no 16-byte units: refused at every width)
    assert _kinds(lib, 128, h, cstride=132, coff=0) == {0}


def _walk(tile, n_res, n):
    """[(unit name, L.Conv, input view, output view, in a residual block)] of the generator under the bf16 policy: the
    dtype of a view is that of the slot the plan allocates (bf16 where the producing unit answers ``bf16_out``)."""
    g_arch = A.cgan_generator_architecture(n_res)
    units, outs = _GanPaintPlan.bf16_policy(g_arch)
    named = _GanPaintPlan._named
    rows, state = [], {"h": tile, "dt": L.F32}

    def walk(layers, prefix, in_res):
        for i, layer in enumerate(layers):
            name = layer[0].lower()
            if name in ("conv", "transp conv"):
                cfg = layer[1]
                tr = name == "transp conv"
                k, s, p, op = cfg["kernel_size"], cfg.get("stride", 1), cfg.get("padding", 0), cfg.get("output_padding", 0)
                h = state["h"]
                ho = (h - 1) * s - 2 * p + k + op if tr else (h + 2 * p - k) // s + 1
                cv = L.Conv(1 if tr else 0, cfg["in_channels"], cfg["out_channels"], k, s, p, op)
                uname = f"{prefix}{i}"
                odt = L.BF16 if named(uname, outs) else L.F32
                vin = L.View(0x10000, n, h, h, cv.cin, cv.cin, 0, state["dt"])
                vout = L.View(0x40000000, n, ho, ho, cv.cout, cv.cout, 0, odt)
                rows.append((uname, cv, vin, vout, in_res, named(uname, units)))
                state["h"], state["dt"] = ho, odt
            elif name == "residual block":
                dt_in = state["dt"]
                walk(layer[1][0], f"{prefix}{i}.res_block.", True)
                assert state["dt"] == dt_in, "a residual block's branch and skip have one element type"
    walk(g_arch, "generator.", False)
    return rows


@pytest.mark.parametrize("tile,n_res", [(64, 2), (512, 9)])
def test_bf16_policy_agrees_with_the_dispatcher(tile, n_res):
    lib = L.load()
    per_batch = []
    for n in BATCHES:
        rows = _walk(tile, n_res, n)
        assert len(rows) == 6 + 2 * n_res and rows[-1][3].h == tile and rows[-1][3].dtype == L.F32
        picked = []
        for uname, cv, vin, vout, in_res, bf16 in rows:
            ok = lib.bp_conv_bf16_supported(C.byref(cv), L.PACK_FWD, C.byref(vin), C.byref(vout)) == 1
            if bf16:
                assert ok, (uname, n)
            else:           # an fp32 layer reads and writes fp32 slots
                assert vin.dtype == L.F32 and vout.dtype == L.F32, uname
            kind = lib.bp_conv_ws_kind(C.byref(cv), L.PACK_FWD, C.byref(vin), C.byref(vout))
            if in_res:
                assert bf16 and vin.dtype == L.BF16 and vout.dtype == L.BF16, uname
                assert kind == 3, (uname, tile, n)          # tile 512: the 128-pixel trunk, two column strips
            picked.append((uname, bf16, vin.dtype, vout.dtype, kind))
        per_batch.append(picked)
    assert all(p == per_batch[0] for p in per_batch), "the kernel choice depends on the batch size"
    bf = [r for r in per_batch[0] if r[1]]
    assert len(bf) == 2 * n_res + 2
    # the layer in front of the blocks reads fp32 and writes bf16, the one behind them reads bf16 and writes fp32
    assert (bf[0][2], bf[0][3]) == (L.F32, L.BF16) and (bf[-1][2], bf[-1][3]) == (L.BF16, L.F32)


def test_policy_of_a_generator_without_residual_blocks_is_empty():
    assert _GanPaintPlan.bf16_policy(A.cgan_generator_architecture(0)) == ((), ())


class _FakeModel:
    tile_size = 64

    def state_dict(self):
        return collections.OrderedDict(a=torch.arange(3.0))


def _bare_painter(paint_dtype=None):
    p = CGANPainter.__new__(CGANPainter)
    p.model = _FakeModel()
    p.stats = {f: {0.0: {"mean": 1.0, "var": 4.0}} for f in ("dm", "pressure")}
    p.tile_size, p.n_res = 64, 1
    p.input_field, p.label_fields = "dm", ["pressure"]
    if paint_dtype is not None:
        p.paint_dtype = paint_dtype
    return p


@pytest.mark.parametrize("paint_dtype", ["bf16", "fp32"])
def test_checkpoint_meta_round_trips_paint_dtype(tmp_path, paint_dtype):
    p = _bare_painter(paint_dtype)
    files = (str(tmp_path / "state"), str(tmp_path / "meta"))
    p.save_state_to_file(files)
    d = CGANPainter._read_meta(files[1])
    assert d["paint_dtype"] == paint_dtype and set(d) == set(CGANPainter.META_KEYS)
    q = CGANPainter.__new__(CGANPainter)
    q._apply_meta(d)
    assert q.paint_dtype == paint_dtype


def test_checkpoint_meta_without_paint_dtype_means_fp32():
    d = _bare_painter()._meta()
    assert d.pop("paint_dtype") == "fp32"           # (a painter that never heard of the key writes fp32)
    q = CGANPainter.__new__(CGANPainter)
    q.paint_dtype = "bf16"
    q._apply_meta(d)
    assert q.paint_dtype == "fp32" and q.tile_size == 64
    d["paint_dtype"] = "fp16"
    with pytest.raises(ValueError):
        q._apply_meta(d)
