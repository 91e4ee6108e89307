"""GPU: the CGAN's training batch assembled on the device -- bp_gather_tiles_gan behind
``DeviceTileAssembler.gather_gan`` / ``CGAN.train_step_assembled`` / ``CGANPainter.use_device_assembly()``.

  1. the kernel against the entry points it stands for (bp_gather_tiles at mode 0 [, bp_tile_minima and a float32
     subtraction], bp_paint_load_cam into views of the same geometry), bit for bit, and what it must leave alone;
  2. the kernel against the float64 transform of the host dataset's raw tiles;
  3. ragged geometry: tile 7, hand-made descriptors, channel offsets and unaligned bases;
  4. refusals, before anything is written;
  5. one training iteration fed in place against ``train_step`` on the same tensors, bit for bit;
  6. ``CGANPainter.train`` on the device path."""
import ctypes as C

import numpy as np
import pytest
import torch

import cgan_paint_ref as R
import gpu_util as G
from baryon_painter_amd import _lib as L
from baryon_painter_amd.utils import data_transforms as T
from baryon_painter_amd.utils.datasets import BAHAMASDataset, DeviceTileAssembler

pytestmark = pytest.mark.gpu
REDSHIFTS = [0.0, 0.5]
NAN = float("nan")


def stacks(grid, seed, n_stack=3):
    """``data=`` of a BAHAMASDataset: seeded positive float32 stacks (n_stack, grid, grid) per field, redshift, slab."""
    rng = np.random.Generator(np.random.PCG64([seed, grid]))
    data = {}
    for f, amp in (("dm", 5.0e3), ("pressure", 0.05)):
        data[f] = {}
        for z in REDSHIFTS:
            data[f][z] = {"100": (rng.random((n_stack, grid, grid), dtype=np.float32) * amp + 0.01 * amp),
                          "150": (rng.random((n_stack, grid, grid), dtype=np.float32) * amp + 0.02 * amp),
                          "mean_100": 0.5 * amp, "mean_150": 0.5 * amp, "var_100": amp * amp / 12,
                          "var_150": amp * amp / 12}
    return data


GRIDS = {16: (64, 4), 48: (96, 2), 64: (128, 2)}          # tile -> (n_grid, n_tile)


def tile_dataset(tile, sub=False):
    grid, n_tile = GRIDS[tile]
    ds = BAHAMASDataset(data=stacks(grid, 5), redshifts=REDSHIFTS, label_fields=["pressure"], n_tile=n_tile, n_stack=2,
                        stack_offset=1, tile_permutations=True, scale_to_SLICS=True, subtract_minimum=sub,
                        fixed_indexing=True)
    assert ds.tile_size == tile
    return ds


def permutation_indices(ds):
    """16 indices in which each slab takes every one of the 8 permutation codes, on changing tiles and redshifts."""
    block = ds.n_sample // 64
    idx = [p * 8 * block + (7 * p + 3) % block for p in range(8)] + \
          [ds.n_sample + p * block + (11 * p + 5) % block for p in range(8)]
    perms = np.array([ds.sample_idx_to_tile_permutation(i) for i in idx])
    assert set(perms[:, 0]) == set(perms[:, 1]) == set(range(8))
    return idx


def cam_rows(ds, idx):
    """(cam (n, 2, 3) float64, aux (n,) float32, redshifts) as CGANPainter forms them for the samples ``idx``."""
    zs = [ds.sample_idx_to_redshift(int(i)) for i in idx]
    sig = lambda f, z: float(np.sqrt(T.interpolate_z(ds.stats[f], z)["var"]))
    cam = np.array([[[sig("dm", z), *R.K], [sig("pressure", z), *R.K]] for z in zs], np.float64)
    return cam, np.asarray(zs, np.float64).astype(np.float32) - np.float32(1.0), zs


class Dst:
    """The four destinations in the geometry of ``_GanPlan``, prefilled with NaN: ``gen`` (n, t, t, 2); ``din``
    (2n, t, t, 4) whose halves are d_real / d_fake_cond; ``x`` (n, 1, t, t)."""

    def __init__(self, n, t):
        self.n, self.t = n, t
        self.gen = torch.full((n, t, t, 2), NAN, device="cuda")
        self.din = torch.full((2 * n, t, t, 4), NAN, device="cuda")
        self.x = torch.full((n, 1, t, t), NAN, device="cuda")
        self.v_gen = L.View(self.gen.data_ptr(), n, t, t, 2, 2, 0)
        self.v_real = L.View(self.din.data_ptr(), n, t, t, 3, 4, 0)
        self.v_fake = L.View(self.din[n:].data_ptr(), n, t, t, 2, 4, 0)

    def views(self):
        return self.v_gen, self.v_real, self.v_fake

    def all_nan(self):
        return bool(torch.isnan(self.gen).all() and torch.isnan(self.din).all() and torch.isnan(self.x).all())


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()


def load_cam(raw, xf, aux, view):
    """bp_paint_load_cam of device tiles (n, 1, t, t) with rows xf (n, 3) [and the aux plane] into ``view``."""
    keep = (G.dev(xf, torch.float64), None if aux is None else G.dev(np.asarray(aux, np.float32).reshape(-1, 1)))
    L.check(L.load().bp_paint_load_cam(L.ptr(raw), 1, L.ptr(keep[0]), L.ptr(keep[1]), 0 if aux is None else 1,
                                       C.byref(view), G.stream()), "paint load cam")
    torch.cuda.synchronize()


def reference(raw_dm, raw_pr, cam, aux, n, t):
    """The existing entry points' composition from raw device tiles (n, 1, t, t): a ``Dst`` filled by bp_paint_load_cam."""
    ref = Dst(n, t)
    for v in (ref.v_gen, L.View(ref.din.data_ptr(), n, t, t, 2, 4, 0), ref.v_fake):
        load_cam(raw_dm, cam[:, 0], aux, v)
    load_cam(raw_pr, cam[:, 1], None, L.View(ref.din.data_ptr(), n, t, t, 1, 4, 2))
    load_cam(raw_pr, cam[:, 1], None, L.View(ref.x.data_ptr(), n, t, t, 1, 1, 0))
    return ref


def gathered_raw(asm, idx, sub):
    """bp_gather_tiles at mode 0 of both fields [, minus the input field's bp_tile_minima in float32]; the descriptors."""
    lib, n, t = L.load(), len(idx), asm.ds.tile_size
    out, desc = [], []
    for f in ("dm", "pressure"):
        rec = asm._descriptors(f, idx)
        assert (rec[2]["mode"] == 0).all()
        d = [up(a) for a in rec]
        raw = torch.empty((n, 1, t, t), device="cuda")
        L.check(lib.bp_gather_tiles(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), n, t, L.ptr(raw), G.stream()), "gather")
        out.append(raw)
        desc.append(d)
    mn = None
    if sub:
        mn = torch.empty(n, device="cuda")
        d = desc[0]
        L.check(lib.bp_tile_minima(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), n, t, L.ptr(mn), G.stream()), "minima")
        out[0] = out[0] - mn[:, None, None, None]
    torch.cuda.synchronize()
    return out[0], out[1], desc, mn


def gather_gan(desc, mn, cam, aux, n, t, dst, views=None, x=None):
    keep = (G.dev(cam, torch.float64), G.dev(aux))
    vg, vr, vf = views or dst.views()
    rc = L.load().bp_gather_tiles_gan(L.ptr(desc[0][0]), L.ptr(desc[0][1]), L.ptr(desc[0][2]), L.ptr(mn),
                                      L.ptr(desc[1][0]), L.ptr(desc[1][1]), L.ptr(desc[1][2]), L.ptr(keep[0]),
                                      L.ptr(keep[1]), n, t, C.byref(vg), C.byref(vr), C.byref(vf),
                                      L.ptr(dst.x) if x is None else x, G.stream())
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def cases():
    """Per (tile, sub): the dataset, 16 indices, the raw gathered tiles, the reference composition and the kernel's
    output -- computed once and left unchanged."""
    cache = {}

    def get(tile, sub):
        if (tile, sub) not in cache:
            ds = tile_dataset(tile, sub)
            asm = DeviceTileAssembler(ds, "cuda:0", mode=None)
            idx = permutation_indices(ds)
            cam, aux, zs = cam_rows(ds, idx)
            raw_dm, raw_pr, desc, mn = gathered_raw(asm, idx, sub)
            ref = reference(raw_dm, raw_pr, cam, aux, len(idx), tile)
            got = Dst(len(idx), tile)
            assert gather_gan(desc, mn, cam, aux, len(idx), tile, got) == L.BP_OK
            cache[(tile, sub)] = dict(ds=ds, asm=asm, idx=idx, cam=cam, aux=aux, zs=zs, ref=ref, got=got, desc=desc, mn=mn)
        return cache[(tile, sub)]
    return get


CASES = [(16, False), (16, True), (48, False), (48, True)]


# ---------------------------------------------------------------------------------------------- 1. the existing kernels
@pytest.mark.parametrize("tile,sub", CASES)
def test_kernel_equals_the_entry_points_it_stands_for(tile, sub, cases):
    c = cases(tile, sub)
    got, ref, n = c["got"], c["ref"], len(c["idx"])
    assert not torch.isnan(ref.gen).any() and not torch.isnan(ref.x).any()
    assert torch.equal(got.gen, ref.gen)
    assert torch.equal(got.din[:n, ..., :3], ref.din[:n, ..., :3])
    assert torch.equal(got.din[n:, ..., :2], ref.din[n:, ..., :2])
    assert torch.equal(got.x, ref.x)
    # the three dm copies and the two pressure copies
    assert torch.equal(got.gen[..., 0], got.din[:n, ..., 0]) and torch.equal(got.gen[..., 0], got.din[n:, ..., 0])
    assert torch.equal(got.x[:, 0], got.din[:n, ..., 2])
    aux = torch.from_numpy(c["aux"]).cuda()[:, None, None].expand(n, tile, tile)
    assert all(torch.equal(a, aux) for a in (got.gen[..., 1], got.din[:n, ..., 1], got.din[n:, ..., 1]))
    # bytes that belong to others: the pad channel of both halves, the fake half's pressure channel
    assert torch.isnan(got.din[..., 3]).all() and torch.isnan(got.din[n:, ..., 2]).all()
    # ... and through the assembler (one packed block, the plan's fill): the same bits

    class Plan:
        n = len(c["idx"])

        def fill(self, fn):
            fn(self.d.v_gen, self.d.v_real, self.d.v_fake, self.d.x)
    plan = Plan()
    plan.d = Dst(n, tile)
    c["asm"].gather_gan(c["idx"], c["cam"], c["aux"], plan)
    torch.cuda.synchronize()
    assert torch.equal(plan.d.gen, got.gen) and torch.equal(plan.d.x, got.x)
    assert torch.equal(plan.d.din.view(torch.int32), got.din.view(torch.int32))       # (NaN bytes included)


# ---------------------------------------------------------------------------------------------- 2. float64
@pytest.mark.parametrize("tile,sub", CASES)
def test_kernel_against_the_float64_transform_of_the_host_tiles(tile, sub, cases):
    """A double logarithm that may differ from NumPy's in its last bit, then ONE rounding to float32: within one float32
    ulp of the rounded reference (the bound of test_gpu_cgan_paint.py::test_load_kernel).  The share of equal values is
    printed."""
    from baryon_painter_amd.painter import CGANPainter
    c = cases(tile, sub)
    ds, got = c["ds"], c["got"]
    dm, pr = got.gen[..., 0].cpu().numpy(), got.x[:, 0].cpu().numpy()
    worst, equal, zeros = 0, [], 0
    for n, i in enumerate(c["idx"]):
        raw_dm, raw_pr, z = CGANPainter._raw(ds, int(i))
        assert raw_dm.dtype == raw_pr.dtype == np.float32 and z == c["zs"][n]
        for g, raw, sigma in ((dm[n], raw_dm, c["cam"][n, 0, 0]), (pr[n], raw_pr, c["cam"][n, 1, 0])):
            d = R.ulps32(g, R.transform(raw, sigma).astype(np.float32))
            worst = max(worst, int(d.max()))
            equal.append((d == 0).mean())
        zero = raw_dm == 0
        zeros += int(zero.sum())
        assert (dm[n][zero] == np.float32(-R.K[1])).all()          # log(0 / sigma + 1) / k0 - k1 = -k1 exactly
    print(f"tile {tile} sub {sub}: max {worst} ulp, {100 * np.mean(equal):.4f} % equal, {zeros} zero pixels")
    assert worst <= 1
    assert zeros >= (len(c["idx"]) if sub else 0)                  # a minimum-subtracted tile touches zero


# ---------------------------------------------------------------------------------------------- 3. ragged geometry
@pytest.mark.parametrize("offset", [False, True], ids=["dense", "offset"])
def test_ragged_geometry(offset):
    """tile 7, n 3: the identity, a flip and a transposing map, by hand over one small stack; with ``offset`` every
    destination starts one channel (the plane: one float) into a wider buffer, so no store is aligned."""
    t, n, H, W = 7, 3, 20, 24
    rng = np.random.default_rng(7)
    stack = (rng.random((4, H, W), dtype=np.float32) * 3.0).astype(np.float32)
    stack[0, 2, 3] = stack[1, 9, 11 + t - 1] = 0.0                # sample 0, output (0, 0): identity at (2, 3) + flip at (9, 11)
    dev = torch.from_numpy(stack).cuda()
    maps = [(0, 1, 0, 0, 0, 1), (0, 1, 0, t - 1, 0, -1), (0, 0, 1, t - 1, -1, 0)]      # (r0, rr, rc, c0, cr, cc)
    origin = [(2, 3), (5, 1), (9, 11)]
    r, c = np.meshgrid(np.arange(t), np.arange(t), indexing="ij")
    scale = {"in": 0.37, "lab": 1.0}
    rec, raw = {}, {}
    for k, (pa, pb) in (("in", (0, 1)), ("lab", (2, 3))):
        tiles = []
        for name, plane, shift in ((k + "100", pa, 0), (k + "150", pb, 1)):
            d = np.zeros(n, DeviceTileAssembler.REC100)
            part = []
            for s in range(n):
                m = maps[(s + shift) % 3]
                y0, x0 = origin[(s + 2 * shift) % 3]
                d[s] = (dev.data_ptr() + 4 * ((plane * H + y0) * W + x0), W) + m + (0,)
                part.append(stack[plane, y0 + m[0] + m[1] * r + m[2] * c, x0 + m[3] + m[4] * r + m[5] * c])
            rec[name] = up(d)
            tiles.append(np.stack(part))
        xf = np.zeros(n, DeviceTileAssembler.XF)
        xf["scale"] = scale[k]
        rec[k + "_xf"] = up(xf)
        s = tiles[0] + tiles[1]
        raw[k] = G.dev((s if scale[k] == 1.0 else np.float32(scale[k]) * s)[:, None])
    assert float(raw["in"].min()) >= 0
    cam = np.array([[[0.8 + 0.1 * s, 4.0, 1.0], [1.7 - 0.2 * s, 3.0, 0.5]] for s in range(n)], np.float64)
    aux = np.array([-1.0, -0.5, 0.25], np.float32)
    cs_gen, cs_d, co = (5, 6, 1) if offset else (2, 4, 0)

    def make():
        gen = torch.full((n, t, t, cs_gen), NAN, device="cuda")
        din = torch.full((2 * n, t, t, cs_d), NAN, device="cuda")
        x = torch.full((n * t * t + 1,), NAN, device="cuda")
        return gen, din, x
    gen, din, x = make()
    rgen, rdin, rx = make()

    def views(gen, din):
        return (L.View(gen.data_ptr(), n, t, t, 2, cs_gen, co), L.View(din.data_ptr(), n, t, t, 3, cs_d, co),
                L.View(din[n:].data_ptr(), n, t, t, 2, cs_d, co))
    xo = 1 if offset else 0
    kc, ka = G.dev(cam, torch.float64), G.dev(aux)
    rcode = L.load().bp_gather_tiles_gan(L.ptr(rec["in100"]), L.ptr(rec["in150"]), L.ptr(rec["in_xf"]), None,
                                         L.ptr(rec["lab100"]), L.ptr(rec["lab150"]), L.ptr(rec["lab_xf"]), L.ptr(kc),
                                         L.ptr(ka), n, t, *(C.byref(v) for v in views(gen, din)),
                                         C.c_void_p(x.data_ptr() + 4 * xo), G.stream())
    torch.cuda.synchronize()
    assert rcode == L.BP_OK
    vg, vr, vf = views(rgen, rdin)
    for v in (vg, L.View(rdin.data_ptr(), n, t, t, 2, cs_d, co), vf):
        load_cam(raw["in"], cam[:, 0], aux, v)
    load_cam(raw["lab"], cam[:, 1], None, L.View(rdin.data_ptr(), n, t, t, 1, cs_d, co + 2))
    load_cam(raw["lab"], cam[:, 1], None, L.View(rx.data_ptr() + 4 * xo, n, t, t, 1, 1, 0))
    assert int(torch.isnan(rgen).sum()) == n * t * t * (cs_gen - 2) and int(torch.isnan(rx).sum()) == 1
    assert int(torch.isnan(rdin).sum()) == n * t * t * (2 * cs_d - 5)
    for a, b in ((gen, rgen), (din, rdin), (x, rx)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))          # values and untouched NaN bytes alike
    assert (gen[0, 0, 0, co] == -1.0) and float(raw["in"][0, 0, 0, 0]) == 0.0  # the planted zero: exactly -k1


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_write_nothing(cases):
    c = cases(16, True)
    n, t, desc, mn, cam, aux = len(c["idx"]), 16, c["desc"], c["mn"], c["cam"], c["aux"]
    dst = Dst(n, t)
    lib, st = L.load(), G.stream()
    kc, ka = G.dev(cam, torch.float64), G.dev(aux)

    def call(args=None, n_=n, t_=t, **views):
        a = [L.ptr(desc[0][0]), L.ptr(desc[0][1]), L.ptr(desc[0][2]), L.ptr(mn), L.ptr(desc[1][0]), L.ptr(desc[1][1]),
             L.ptr(desc[1][2]), L.ptr(kc), L.ptr(ka)]
        v = dict(gen=dst.v_gen, real=dst.v_real, fake=dst.v_fake)
        v.update(views)
        tail = [None if v[k] is None else C.byref(v[k]) for k in ("gen", "real", "fake")] + [L.ptr(dst.x)]
        for i in (args or ()):
            if i < 9:
                a[i] = None
            else:
                tail[i - 9] = None
        rc = lib.bp_gather_tiles_gan(*a, n_, t_, *tail, st)
        torch.cuda.synchronize()
        assert dst.all_nan()
        return rc

    def alter(v, **kw):
        w = L.View(v.ptr, v.n, v.h, v.w, v.c, v.cstride, v.coff, v.dtype)
        for k, val in kw.items():
            setattr(w, k, val)
        return w
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12):             # every pointer but in_minima (3)
        assert call(args=[i]) == L.BP_EINVAL, i
    assert call(n_=0) == L.BP_EINVAL and call(n_=-1) == L.BP_EINVAL and call(t_=0) == L.BP_EINVAL
    assert call(n_=n + 1) == L.BP_EINVAL and call(t_=t + 1) == L.BP_EINVAL
    for name, v in (("gen", dst.v_gen), ("real", dst.v_real), ("fake", dst.v_fake)):
        for field in ("n", "h", "w"):
            for step in (-1, 1):
                assert call(**{name: alter(v, **{field: getattr(v, field) + step})}) == L.BP_EINVAL, (name, field)
        assert call(**{name: alter(v, c=v.c - 1)}) == L.BP_EINVAL, name
        assert call(**{name: alter(v, c=v.c + 1, cstride=4)}) == L.BP_EINVAL, name
        assert call(**{name: alter(v, dtype=L.BF16)}) == L.BP_EUNSUPPORTED, name
    # and the call the refusals were variations of goes through (in_minima = NULL too)
    assert gather_gan(desc, None, cam, aux, n, t, dst) == L.BP_OK and not torch.isnan(dst.gen).any()


# ---------------------------------------------------------------------------------------------- 5. one iteration
def _adam(m):
    return (torch.optim.Adam(m.g_parameters(), lr=5e-5, betas=(0.5, 0.999)),
            torch.optim.Adam(m.d_parameters(), lr=5e-5, betas=(0.5, 0.999)))


def test_one_iteration_filled_in_place_equals_train_step_bit_for_bit():
    """``_GanPlan`` is deterministic (fixed reduction orders, no atomics): the same inputs give the same bits, so no
    tolerance is involved."""
    from baryon_painter_amd.models.cgan import CGAN
    tile, batch = 64, 2
    ds = tile_dataset(tile)
    asm = DeviceTileAssembler(ds, "cuda:0", mode=None)
    idx = [permutation_indices(ds)[k] for k in (3, 12)]
    cam, aux, zs = cam_rows(ds, idx)
    assert zs[0] != zs[1]
    raw_dm, raw_pr, _, _ = gathered_raw(asm, idx, False)
    y, x = torch.empty((batch, 1, tile, tile), device="cuda"), torch.empty((batch, 1, tile, tile), device="cuda")
    load_cam(raw_dm, cam[:, 0], None, L.View(y.data_ptr(), batch, tile, tile, 1, 1, 0))
    load_cam(raw_pr, cam[:, 1], None, L.View(x.data_ptr(), batch, tile, tile, 1, 1, 0))
    torch.manual_seed(0)
    m = CGAN(tile_size=tile, device="cuda:0", n_res=1)
    m.train(True)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert any("weight_u" in k for k in state) and any("running_mean" in k for k in state)

    def run(step):
        m.load_state_dict(state)
        assert all(torch.equal(v, state[k]) for k, v in m.state_dict().items())
        opt_g, opt_d = _adam(m)
        cap = {}
        losses = step(opt_g, opt_d, cap)
        torch.cuda.synchronize()
        return ({k: v.clone() for k, v in losses.items()}, cap,
                {k: v.detach().clone() for k, v in m.state_dict().items()})
    l0, c0, s0 = run(lambda og, od, cap: m.train_step(x, y, torch.tensor(zs, dtype=torch.float32), og, od, capture=cap))
    l1, c1, s1 = run(lambda og, od, cap: m.train_step_assembled(
        lambda plan: asm.gather_gan(idx, cam, aux, plan), batch, og, od, capture=cap))
    assert set(l0) == set(l1) == {"D", "G_adv", "G_perceptual"}
    for k in l0:
        assert np.isfinite(float(l0[k])) and torch.equal(l0[k], l1[k]), (k, float(l0[k]), float(l1[k]))
    for part in ("d", "g"):
        assert len(c0[part]) > 3 and set(c0[part]) == set(c1[part])
        for k in c0[part]:
            assert float(c0[part][k].abs().sum()) > 0 and torch.equal(c0[part][k], c1[part][k]), (part, k)
    moved = 0
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
        moved += int(not torch.equal(s0[k], state[k]))
    assert moved > 10                                              # the step did step


# ---------------------------------------------------------------------------------------------- 6. the painter
def test_painter_trains_from_the_assembler(monkeypatch):
    from baryon_painter_amd.painter import CGANPainter
    tile, batch = 64, 2
    ds = tile_dataset(tile)
    torch.manual_seed(1)
    p = CGANPainter(training_data_set=ds, tile_size=tile, compute_device="cuda:0", n_res=1)
    state = {k: v.detach().clone() for k, v in p.model.state_dict().items()}
    assert getattr(p, "device_assembler", None) is None
    p.use_device_assembly()
    assert isinstance(p.device_assembler, DeviceTileAssembler) and p.device_assembler.mode is None

    def host_path(*a, **k):
        raise AssertionError("the host path was taken")
    with monkeypatch.context() as mp:
        mp.setattr(CGANPainter, "transform", host_path)
        mp.setattr(ds, "get_stack", host_path)
        log = p.train(n_iter=3, batch_size=batch)
    assert len(log) == 3 and all(set(row) == {"D", "G_adv", "G_perceptual"} for row in log)
    assert all(isinstance(v, float) and np.isfinite(v) for row in log for v in row.values())
    # the first iteration is train_step_assembled on the indices default_rng(0) draws, from the same weights
    m = p.model
    m.load_state_dict(state)
    m.train(True)
    idx = np.random.default_rng(0).integers(0, len(ds), batch)
    cam, aux, _ = cam_rows(ds, idx)
    opt_g, opt_d = _adam(m)
    first = m.train_step_assembled(lambda plan: p.device_assembler.gather_gan(idx, cam, aux, plan), batch, opt_g, opt_d)
    assert {k: float(v) for k, v in first.items()} == log[0]
    # a painter without use_device_assembly() still trains through the old loop
    torch.manual_seed(1)
    q = CGANPainter(training_data_set=ds, tile_size=tile, compute_device="cuda:0", n_res=1)
    calls = []
    transform = CGANPainter.transform
    monkeypatch.setattr(CGANPainter, "transform", lambda self, x, f, z: (calls.append(f), transform(self, x, f, z))[1])
    host = q.train(n_iter=1, batch_size=batch)
    assert calls == ["dm", "pressure"] * batch and len(host) == 1 and set(host[0]) == set(log[0])
    print("first iteration, device path:", log[0], "host path:", host[0])
    assert all(np.isfinite(v) for v in host[0].values())
