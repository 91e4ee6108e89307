"""CPU: what the CGAN's device paint path rests on and that needs no GPU -- the float64 restatement of its transform
(tests/cgan_paint_ref.py), the batch-size independence of the kernels the dispatcher picks for the generator's layers,
and the metadata half of a (state, meta) checkpoint."""
import collections
import ctypes as C
import pickle

import numpy as np
import torch

import cgan_paint_ref as R
from baryon_painter_amd import _lib as L
from baryon_painter_amd.models import arch as A
from baryon_painter_amd.painter import CGANPainter


def test_reference_transform_known_answers_and_round_trip():
    e = np.e
    # sigma = 2: log(x / 2 + 1) = 0, 1, 4, 8 -> / 4 - 1 = -1, -0.75, 0, 1 (the tanh range)
    x = np.array([0.0, 2.0 * (e - 1), 2.0 * (e ** 4 - 1), 2.0 * (e ** 8 - 1)])
    assert np.allclose(R.transform(x, 2.0), [-1.0, -0.75, 0.0, 1.0], atol=1e-14)
    assert np.allclose(R.inverse(np.array([-1.0, -0.75]), 0.5), [0.0, 0.5 * (e - 1)], atol=1e-15)
    # the painter's own host transform is the same expression (rounded to float32 on the way in)
    p = CGANPainter.__new__(CGANPainter)
    p.stats = {"dm": {0.0: {"mean": 1.0, "var": 4.0}}, "pressure": {0.0: {"mean": 1.0, "var": 0.25}}}
    assert CGANPainter.K == R.K
    assert np.array_equal(p.transform(x, "dm", 0.0), R.transform(x, 2.0).astype(np.float32))
    assert np.array_equal(p.inverse_transform(x[:3] / 10 - 1, "pressure", 0.0), R.inverse(x[:3] / 10 - 1, 0.5))
    # Round trip.  The shift by k1 = 1 costs an absolute 2^-53 in the log domain, times k0 = 4 on the way back, which
    # is 4.4e-16 * (x / sigma + 1) / (x / sigma) of x: below 1e-12 for x >= 1e-3 sigma, the range drawn here.
    rng = np.random.default_rng(0)
    for sigma in (0.03, 1.0, 17.0):
        x = sigma * 10.0 ** rng.uniform(-3, 4, 4000)
        back = R.inverse(R.transform(x, sigma), sigma)
        assert np.abs(back / x - 1).max() <= 1e-12, (sigma, np.abs(back / x - 1).max())


def test_reference_load_and_store_layouts():
    rng = np.random.default_rng(1)
    raw = rng.uniform(0, 5, (2, 1, 3, 4))
    xf = np.array([[2.0, 4.0, 1.0], [0.5, 4.0, 1.0]])
    aux = np.array([[-0.7], [0.2]])
    out = R.load(raw, xf, aux)
    assert out.shape == (2, 3, 4, 2)
    for n in range(2):
        assert np.array_equal(out[n, :, :, 0], R.transform(raw[n, 0], xf[n, 0]))
        assert (out[n, :, :, 1] == aux[n, 0]).all()
    y = rng.uniform(-1, 1, (2, 3, 4, 1))
    xo = np.array([[4.0, 1.0, 0.3], [4.0, 1.0, 2.0]])
    st = R.store(y, xo)
    assert st.shape == (2, 1, 3, 4)
    for n in range(2):
        assert np.array_equal(st[n, 0], R.inverse(y[n, :, :, 0], xo[n, 2]))
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(-3.0) == 2.0 ** -22
    assert R.ulps32(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1


def _generator_convs(tile, n_res):
    """(L.Conv, input h, output h) of every convolution of the generator, in order, walking its layer table."""
    out, h = [], tile

    def walk(layers):
        nonlocal h
        for layer in layers:
            name = layer[0].lower()
            if name in ("conv", "transp conv"):
                cfg = layer[1]
                tr = name == "transp conv"
                k, s, p, op = cfg["kernel_size"], cfg.get("stride", 1), cfg.get("padding", 0), cfg.get("output_padding", 0)
                ho = (h - 1) * s - 2 * p + k + op if tr else (h + 2 * p - k) // s + 1
                out.append((L.Conv(1 if tr else 0, cfg["in_channels"], cfg["out_channels"], k, s, p, op), h, ho))
                h = ho
            elif name == "residual block":
                walk(layer[1][0])
    walk(A.cgan_generator_architecture(n_res))
    return out


def test_generator_kernel_choice_does_not_depend_on_the_batch_size():
    """A tile's bits do not depend on the batch it is painted in only if every layer runs the same kernel at every batch
    size.  bp_conv_kernel_id takes the layer alone; the one forward kernel that is picked by the VIEWS of a layer
    (bp_conv_ws_kind: the weights-stationary trunk kernel) is asked with views of each batch size.  Both are host
    arithmetic: the view pointers are never dereferenced."""
    lib = L.load()
    for tile, n_res in ((64, 1), (64, 9), (512, 9)):
        convs = _generator_convs(tile, n_res)
        assert len(convs) == 6 + 2 * n_res and convs[-1][2] == tile
        for cv, hi, ho in convs:
            ids, kinds = set(), set()
            for n in (1, 3, 4, 11, 64):
                ids.add(lib.bp_conv_kernel_id(C.byref(cv), L.PACK_FWD))
                vin = L.View(0x10000, n, hi, hi, cv.cin, cv.cin, 0, L.F32)
                vout = L.View(0x20000, n, ho, ho, cv.cout, cv.cout, 0, L.F32)
                kinds.add(lib.bp_conv_ws_kind(C.byref(cv), L.PACK_FWD, C.byref(vin), C.byref(vout)))
            assert len(ids) == 1 and min(ids) > 0, (tile, cv.cin, cv.cout, cv.k, ids)
            assert len(kinds) == 1, (tile, cv.cin, cv.cout, cv.k, kinds)


class _FakeModel:
    tile_size = 64

    def state_dict(self):
        return collections.OrderedDict(a=torch.arange(3.0), b=torch.ones(2, 2))


def _bare_painter():
    p = CGANPainter.__new__(CGANPainter)
    p.model = _FakeModel()
    p.stats = collections.OrderedDict(
        (f, collections.OrderedDict((z, {"mean": 1.0, "var": v * (1 + z)}) for z in (0.0, 0.5, 1.0)))
        for f, v in (("dm", 4.0), ("pressure", 0.25)))
    p.tile_size, p.n_res = 64, 1
    p.input_field, p.label_fields = "dm", ["pressure"]
    return p


def test_checkpoint_meta_round_trip(tmp_path):
    p = _bare_painter()
    files = (str(tmp_path / "state"), str(tmp_path / "meta"))
    p.save_state_to_file(files)
    d = CGANPainter._read_meta(files[1])
    assert set(d) == set(CGANPainter.META_KEYS)
    q = CGANPainter.__new__(CGANPainter)
    q._apply_meta(d)
    assert q.stats == p.stats and q.K == CGANPainter.K and (q.tile_size, q.n_res) == (64, 1)
    assert q.input_field == "dm" and q.label_fields == ["pressure"]
    assert q.can_paint_stream(0.3) and q.can_paint_stream(7.0)
    x = np.array([0.1, 2.0, 30.0])
    assert np.array_equal(q.transform(x, "dm", 0.25), p.transform(x, "dm", 0.25))
    prm = q._cam_parameters(np.array([0.25, 3.0]))
    assert prm["xf_in"].shape == prm["xf_out"].shape == (2, 3) and prm["aux"].dtype == np.float32
    assert np.array_equal(prm["xf_in"][:, 0], [q._sigma("dm", 0.25), q._sigma("dm", 3.0)])
    assert np.array_equal(prm["xf_out"][:, 2], [q._sigma("pressure", 0.25), q._sigma("pressure", 3.0)])
    assert np.array_equal(prm["xf_in"][:, 1:], [[4.0, 1.0]] * 2) and np.array_equal(prm["xf_out"][:, :2], [[4.0, 1.0]] * 2)
    assert np.array_equal(prm["aux"], np.array([0.25, 3.0], np.float32) - np.float32(1))
    state = torch.load(files[0])
    assert list(state) == ["a", "b"] and torch.equal(state["a"], torch.arange(3.0))
    with open(files[1], "rb") as f:
        assert pickle.load(f)["tile_size"] == 64           # (dill writes what pickle reads: plain containers only)
    d.pop("stats")
    try:
        q._apply_meta(d)
    except ValueError:
        pass
    else:
        raise AssertionError("metadata without statistics must be refused")


def test_single_path_checkpoint_is_a_plain_state_dict(tmp_path):
    p = _bare_painter()
    path = str(tmp_path / "only_state")
    p.save_state_to_file(path)
    state = torch.load(path)
    assert isinstance(state, dict) and list(state) == ["a", "b"] and all(isinstance(v, torch.Tensor) for v in state.values())
    assert not (tmp_path / "meta").exists() and [f.name for f in tmp_path.iterdir()] == ["only_state"]
    # a painter without statistics has no device (or host) transform
    q = CGANPainter.__new__(CGANPainter)
    q.stats, q.input_field, q.label_fields = None, "dm", ["pressure"]
    assert not q.can_paint_stream()
    try:
        q._cam_parameters(np.zeros(1))
    except NotImplementedError:
        pass
    else:
        raise AssertionError("no statistics, no device transform")
