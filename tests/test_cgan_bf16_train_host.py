"""CPU: what ``train_dtype="bf16"`` of the CGAN rests on and that needs no GPU -- the constructor's refusals, the
``train_dtype`` key of a checkpoint's metadata, which widths the output-stationary bf16 weight gradient takes
(bp_conv_backward_weight_plan is host arithmetic: the view pointers are looked at for their alignment only), the number
of partial images of the GPU test's cases, and the element type of every layer's views under the training policy."""
import collections
import ctypes as C

import pytest
import torch

from baryon_painter_amd import _lib as L
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.models.cgan import CGAN, _GanPlan
from baryon_painter_amd.painter import CGANPainter

BATCHES = (1, 3, 4, 11, 64)
TRUNK = L.Conv(0, 128, 128, 3, 1, 1, 0)
# (n, h, w) of the strip weight-gradient cases of tests/test_gpu_cgan_bf16_train_ops.py -> (bands per image, strips)
STRIP_CASES = {(1, 1, 128): (1, 2), (2, 9, 128): (2, 2), (3, 20, 192): (4, 3), (2, 37, 256): (8, 4), (1, 128, 128): (16, 2)}


def _plan(lib, n, h, w, cstride=128, coff=0):
    """(rc, family name, nsplit) of the trunk layer's weight gradient on bf16 views."""
    x = L.View(0x10000, n, h, w, 128, cstride, coff, L.BF16)
    y = L.View(0x4000000, n, h, w, 128, cstride, coff, L.BF16)
    out = (C.c_int32 * 4)()
    rc = lib.bp_conv_backward_weight_plan(C.byref(TRUNK), C.byref(x), C.byref(y), L.IMPL_BF16, out)
    need = lib.bp_conv_backward_weight_workspace(C.byref(TRUNK), C.byref(x), C.byref(y))
    assert rc == L.BP_OK and need >= out[1] * 9 * out[2] * out[3] * 4, (n, h, w, rc, need, list(out))
    return L.WGRAD_FAMILIES[out[0]], out[1]


# ---------------------------------------------------------------------------------------------------- constructor
def test_unknown_train_dtype_is_a_value_error_before_any_device_is_touched():
    with pytest.raises(ValueError, match="train_dtype"):
        CGAN(tile_size=64, device="cpu", train_dtype="fp16")
    with pytest.raises(ValueError, match="train_dtype"):
        CGAN(tile_size=64, device="cuda:0", n_res=1, train_dtype="bfloat16")


def test_data_parallel_bf16_training_is_refused_in_the_constructor():
    with pytest.raises(NotImplementedError, match="bf16"):
        CGAN(tile_size=64, device="cpu", sync=object(), train_dtype="bf16")
    # (fp32 with a communicator goes on as before: the next refusal is the missing device)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        CGAN(tile_size=64, device="cpu", sync=object(), train_dtype="fp32")


# ---------------------------------------------------------------------------------------------------- checkpoint meta
class _FakeModel:
    tile_size = 64

    def state_dict(self):
        return collections.OrderedDict(a=torch.arange(3.0))


def _bare_painter(train_dtype=None):
    p = CGANPainter.__new__(CGANPainter)
    p.model = _FakeModel()
    p.stats = {f: {0.0: {"mean": 1.0, "var": 4.0}} for f in ("dm", "pressure")}
    p.tile_size, p.n_res = 64, 1
    p.input_field, p.label_fields = "dm", ["pressure"]
    if train_dtype is not None:
        p.train_dtype = train_dtype
    return p


@pytest.mark.parametrize("train_dtype", ["bf16", "fp32"])
def test_checkpoint_meta_round_trips_train_dtype(tmp_path, train_dtype):
    p = _bare_painter(train_dtype)
    files = (str(tmp_path / "state"), str(tmp_path / "meta"))
    p.save_state_to_file(files)
    d = CGANPainter._read_meta(files[1])
    assert d["train_dtype"] == train_dtype and d["paint_dtype"] == "fp32" and set(d) == set(CGANPainter.META_KEYS)
    q = CGANPainter.__new__(CGANPainter)
    q._apply_meta(d)
    assert q.train_dtype == train_dtype and q.paint_dtype == "fp32"


def test_checkpoint_meta_without_train_dtype_means_fp32():
    assert CGANPainter.OPTIONAL_META["train_dtype"] == "fp32" and "train_dtype" in CGANPainter.META_KEYS
    d = _bare_painter()._meta()
    assert d.pop("train_dtype") == "fp32"           # (a painter that never heard of the key writes fp32)
    q = CGANPainter.__new__(CGANPainter)
    q.train_dtype = "bf16"
    q._apply_meta(d)
    assert q.train_dtype == "fp32" and q.tile_size == 64
    d["train_dtype"] = "fp16"
    with pytest.raises(ValueError):
        q._apply_meta(d)


# ---------------------------------------------------------------------------------------------------- weight-gradient plan
@pytest.mark.parametrize("h", [8, 128])
def test_strip_widths_go_to_the_stationary_kernel_at_every_batch_size(h):
    lib = L.load()
    for n in BATCHES:
        for w in (128, 192, 256):
            assert _plan(lib, n, h, w)[0] == "ws_bf16", (n, w)
            assert _plan(lib, n, h, w, 136, 8)[0] == "ws_bf16", (n, w)
        for w in (32, 64):                                  # (the widths of before)
            assert _plan(lib, n, h, w)[0] == "ws_bf16", (n, w)
        for w in (96, 320, 512):                            # no multiple of 64, or more than four strips
            assert _plan(lib, n, h, w)[0] == "bf16_tiled", (n, w)


def test_the_option_switches_every_width_back_to_the_tiled_kernel():
    lib = L.load()
    try:
        assert lib.bp_set_option(b"BP_BF16_WGRAD_WS", 0) == L.BP_OK
        for n in BATCHES:
            for w in (32, 64, 96, 128, 192, 256, 320, 512):
                assert _plan(lib, n, 8, w)[0] == "bf16_tiled", (n, w)
        assert lib.bp_set_option(b"BP_BF16_WGRAD_WS", 1) == L.BP_OK
        assert _plan(lib, 2, 8, 128)[0] == "ws_bf16"
    finally:
        lib.bp_set_option(b"BP_BF16_WGRAD_WS", -1)
    assert _plan(lib, 2, 8, 128)[0] == "ws_bf16" and _plan(lib, 2, 8, 64)[0] == "ws_bf16"


def test_partial_images_of_the_gpu_cases_are_bands_times_strips():
    """A work item is image-band x strip and writes one partial image: nsplit = n x bands x strips.  The GPU cases cover
    one, two and three or more bands per image and two, three and four strips."""
    lib = L.load()
    for (n, h, w), (bands, strips) in STRIP_CASES.items():
        assert strips == w // 64
        for layout in ((128, 0), (136, 8)):
            assert _plan(lib, n, h, w, *layout) == ("ws_bf16", n * bands * strips), (n, h, w)
    bands = {b for b, _ in STRIP_CASES.values()}
    assert 1 in bands and 2 in bands and max(bands) >= 3
    assert {s for _, s in STRIP_CASES.values()} == {2, 3, 4}


# ---------------------------------------------------------------------------------------------------- training policy
def _walk(tile, n_res, n):
    """[(unit name, L.Conv, input view, output view, in a residual block, runs in bf16)] of the generator under the
    training policy: bf16 between the entry cast in front of the first block and the exit cast behind the last one."""
    g_arch = A.cgan_generator_architecture(n_res)
    convs, first, behind = _GanPlan.bf16_policy(g_arch)
    rows, state = [], {"h": tile, "dt": L.F32}

    def walk(layers, prefix, in_res):
        for i, layer in enumerate(layers):
            name = layer[0].lower()
            uname = f"{prefix}{i}"
            if uname == first:
                state["dt"] = L.BF16            # (the entry cast)
            if uname == behind:
                state["dt"] = L.F32             # (the exit cast)
            if name in ("conv", "transp conv"):
                cfg = layer[1]
                tr = name == "transp conv"
                k, s, p, op = cfg["kernel_size"], cfg.get("stride", 1), cfg.get("padding", 0), cfg.get("output_padding", 0)
                h = state["h"]
                ho = (h - 1) * s - 2 * p + k + op if tr else (h + 2 * p - k) // s + 1
                cv = L.Conv(1 if tr else 0, cfg["in_channels"], cfg["out_channels"], k, s, p, op)
                bf16 = bool(convs) and uname.startswith(convs)
                odt = L.BF16 if bf16 else L.F32
                vin = L.View(0x10000, n, h, h, cv.cin, cv.cin, 0, state["dt"])
                vout = L.View(0x40000000, n, ho, ho, cv.cout, cv.cout, 0, odt)
                rows.append((uname, cv, vin, vout, in_res, bf16))
                state["h"], state["dt"] = ho, odt
            elif name == "residual block":
                dt_in = state["dt"]
                walk(layer[1][0], f"{uname}.res_block.", True)
                assert state["dt"] == dt_in == L.BF16, "a residual block's branch and skip are bf16"
    walk(g_arch, "generator.", False)
    return rows


@pytest.mark.parametrize("tile,n_res", [(64, 2), (256, 1), (512, 9)])
def test_training_policy_marks_exactly_the_residual_convolutions(tile, n_res):
    lib = L.load()
    for n in (1, 6, 64):
        rows = _walk(tile, n_res, n)
        assert len(rows) == 6 + 2 * n_res and rows[-1][3].h == tile
        assert [r[0] for r in rows if r[5]] == [r[0] for r in rows if r[4]] and sum(r[5] for r in rows) == 2 * n_res
        for uname, cv, vin, vout, in_res, bf16 in rows:
            if bf16:
                assert vin.dtype == L.BF16 and vout.dtype == L.BF16, uname
                for d, (a, b) in ((L.PACK_FWD, (vin, vout)), (L.PACK_BWD, (vout, vin))):
                    assert lib.bp_conv_bf16_supported(C.byref(cv), d, C.byref(a), C.byref(b)) == 1, (uname, d)
                out = (C.c_int32 * 4)()
                assert lib.bp_conv_backward_weight_plan(C.byref(cv), C.byref(vin), C.byref(vout), L.IMPL_BF16, out) == L.BP_OK
                want = "ws_bf16" if tile // 4 in (32, 64, 128, 192, 256) else "bf16_tiled"
                assert L.WGRAD_FAMILIES[out[0]] == want, (uname, tile, n)
            else:               # every other layer reads and writes fp32, biased boundary layers included
                assert vin.dtype == L.F32 and vout.dtype == L.F32, uname


def test_policy_of_a_generator_without_residual_blocks_is_empty():
    assert _GanPlan.bf16_policy(A.cgan_generator_architecture(0)) == ((), None, None)
