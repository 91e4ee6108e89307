"""Cases that make every persistent forward / data-gradient kernel walk three and four tiles, and the host arithmetic
behind them (plain module, no test in here).

Most fp32 forward and data-gradient kernels cap their grid and let each workgroup walk the tile sequence: the next tile
is fetched into registers, with a bit mask of the elements inside the image, while the current one is multiplied, and is
committed to LDS behind a barrier.  tests/conv_sweep.py reaches the second step of such a walk for 2 workgroups of a few
kernels, through the statistics entry points only, with the same clip mask at every step.  The cases here reach, through
the plain entry points,
  * the steady state: the registers fetched for tile t + 1 are consumed while the fetch of t + 2 is issued (three tiles);
  * a tile clipped at the right or bottom edge followed, in the same walk, by a full one (a stale mask shows);
  * walks that cross from one image to the next, with a ragged remainder (tiles % grid != 0).
Geometry of every case: 3 x 3 tiles per image, extent 2 TH + 1 by 2 TW + 1 in the tile's own coordinates (output pixels
or, for the transposed forms, the phase grid): full, x-clipped, y-clipped and corner tiles.  Nine tiles per image are
coprime with every cap (powers of two), so a workgroup meets another kind of tile at each step.  n is the smallest batch
at which every workgroup walks at least three tiles and some walk one more: for the grid-stride kernels 9 n > 3 cap and
9 n % cap != 0, for the kernels that walk contiguous runs the smallest n whose shortest (the last) run has three tiles
and is shorter than the others.  test_walk_sweep_host.py checks each record against the library's own answers without a
GPU; test_gpu_walk_sweep.py runs the cases.
"""
import collections
import os

import numpy as np
import torch

import conv_sweep as S

# One record per walking kernel.  kid: bp_conv_kernel_id (None: the bf16 kernels have none); th x tw: the tile, in output
# pixels or (phase > 1) pixels of the phase grid, i.e. ceil(extent / phase); cap: the most workgroups (per produced-channel
# block); walk: "stride" (tile += grid) or "runs" (a contiguous run of per_block tiles per workgroup), min_per: the
# shortest run the launch ever plans; vec_out: the kernel stores 16 bytes at a time and BP_IMPL_MFMA refuses any other
# produced view (BP_IMPL_AUTO takes the direct kernel there); src: where each number was read.
Inst = collections.namedtuple("Inst", "kid th tw phase cap walk min_per vec_out src")
INST = {
    "stem_forward": Inst(700000, 8, 64, 1, 2048, "stride", 0, False, "conv_stem.hip:24 TH, TW; :324 stem_grid; :110 walk"),
    "flat_k7": Inst(710000, 8, 64, 1, 512, "stride", 0, False, "conv_flat.hip:23 TH, TW; :203 flat_grid; :115 walk"),
    "flat_h7": Inst(750000, 8, 32, 1, 256, "stride", 0, True, "conv_flat.hip:1038 HTH, HTW; :1257 flat_g4_grid; :1144 walk; :1248"),
    "flat_t4": Inst(720000, 8, 16, 2, 512, "stride", 0, True, "conv_flat.hip:276 TTH, TTW; :480 flat_grid; :367 walk; :471"),
    "flat_t64": Inst(740000, 8, 16, 2, 256, "stride", 0, True, "conv_flat.hip:769 WTH, WTW; :1007 flat_g4_grid; :864 walk; :998"),
    "flat_g4": Inst(730000, 4, 16, 1, 256, "stride", 0, True, "conv_flat.hip:504 GTW, :525 GTH (64 channels: 4); :742; :600 walk; :733"),
    "enc_fwd": Inst(760000, 4, 16, 1, 512, "stride", 0, False, "conv_enc.hip:40 EF_R; :637 enc_fwd_grid (256 x 2); :117 walk"),
    "enc_dgrad": Inst(770000, 4, 16, 4, 1024, "stride", 0, False, "conv_enc.hip:209 ED_RQ; :707-712 (256 x 4); :270 walk"),
    "enc0_fwd_1": Inst(780001, 8, 32, 1, 2048, "stride", 0, False, "conv_enc.hip:347 E0_R, E0_W; :647 enc0_fwd_grid; :418 walk"),
    "enc0_fwd_2": Inst(780002, 8, 32, 1, 2048, "stride", 0, False, "conv_enc.hip:347 E0_R, E0_W; :647 enc0_fwd_grid; :418 walk"),
    # igemm_wres_kernel, four waves: tile_geom(8, ...) = 8 rows x 16 columns, 256 CUs x 2 workgroups / channel blocks (1)
    "igemm_wres": Inst(416212, 8, 16, 1, 512, "runs", 1, False, "conv_igemm.hip:1230-1241 NW 4, tw; :1509-1518 runs; :972 walk"),
    # igemm_bf16_p_kernel: BH x 16 TPR = 8 x 32 pixels of one phase; 512 / (channel blocks x phases) workgroups, at least 64
    "igemm_bf16_p": Inst(None, 8, 32, 1, 512, "runs", 4, False, "conv_bf16.hpp:741-744 TM, BH; :846-850, :860 runs of >= 4"),
    # ... FUSE: all four phases of a stride-2 transposed form per tile of the phase grid
    "igemm_bf16_pf": Inst(None, 8, 32, 2, 512, "runs", 2, False, "conv_bf16.hpp:766-777 fuse; :852-856 runs of >= 2"),
}

# Environment switches that move a layer of the table to another kernel or change a cap.  The library reads them once per
# process; with one set, the arithmetic below describes another launch than the one that runs.
SWITCHES = ("BP_FLAT_GRID", "BP_FLATG_GRID", "BP_STEM_GRID", "BP_ENC_WGS", "BP_ENC0_WGS", "BP_WRES_GRID",
            "BP_NOFLAT", "BP_NOFLATG", "BP_NOFLATW", "BP_NOFLATH", "BP_FLATG_THIN", "BP_FLATW_THIN", "BP_NOSTEM", "BP_NOENC",
            "BP_NOENC0", "BP_IGEMM_NOWRES", "BP_IGEMM_WRESALL", "BP_WRES_NO4", "BP_BF16_NOPERSIST", "BP_BF16_NOFUSE",
            "BP_BF16_PALL")


def require_production_environment():
    """Raises (a skip would hide the sweep) if a switch is set."""
    found = [s for s in SWITCHES if s in os.environ]
    if found:
        raise RuntimeError("the walk sweep describes the production launch: unset %s" % ", ".join(found))


FWD, BWD = 0, 1                         # direction: forward / data gradient (L.PACK_FWD / L.PACK_BWD)

# (tag, inst, direction, impl the case is listed for, module layer, (n, h, w) of the module input)
#                                       (transposed, cin, cout, k, stride, pad, out_pad)
Entry = collections.namedtuple("Entry", "tag inst direction impl case")
_TABLE = [
    ("stem:f", "stem_forward", FWD, "mfma", (0, 3, 16, 5, 1, 2, 0), (683, 17, 129)),
    ("flat_k7:f", "flat_k7", FWD, "mfma", (0, 8, 16, 7, 1, 3, 0), (171, 17, 129)),
    ("flat_k7:d", "flat_k7", BWD, "mfma", (0, 16, 8, 7, 1, 3, 0), (171, 17, 129)),
    ("flat_h7:f", "flat_h7", FWD, "mfma", (0, 16, 8, 7, 1, 3, 0), (86, 17, 65)),
    ("flat_h7:d", "flat_h7", BWD, "mfma", (0, 8, 16, 7, 1, 3, 0), (86, 17, 65)),
    ("flat_t4:f", "flat_t4", FWD, "mfma", (1, 32, 16, 4, 2, 1, 0), (171, 17, 33)),
    ("flat_t4:d", "flat_t4", BWD, "mfma", (0, 16, 32, 4, 2, 1, 0), (171, 33, 65)),         # (odd extents: phase 1 is one short)
    ("flat_t64:f", "flat_t64", FWD, "mfma", (1, 64, 32, 4, 2, 1, 0), (86, 17, 33)),
    ("flat_t64:d", "flat_t64", BWD, "mfma", (0, 32, 64, 4, 2, 1, 0), (86, 33, 65)),
    ("flat_g4:f", "flat_g4", FWD, "mfma", (0, 32, 64, 4, 2, 1, 0), (86, 18, 66)),
    ("flat_g4:d", "flat_g4", BWD, "mfma", (1, 64, 32, 4, 2, 1, 0), (86, 9, 33)),
    ("enc_fwd:f", "enc_fwd", FWD, "mfma", (0, 8, 16, 8, 4, 2, 0), (171, 36, 132)),
    ("enc_fwd:d", "enc_fwd", BWD, "mfma", (1, 16, 8, 8, 4, 2, 0), (171, 9, 33)),
    ("enc_dgrad:f", "enc_dgrad", FWD, "mfma", (1, 16, 8, 8, 4, 2, 0), (342, 9, 33)),
    ("enc_dgrad:d", "enc_dgrad", BWD, "mfma", (0, 8, 16, 8, 4, 2, 0), (342, 33, 129)),     # (33 = 4 x 8 + 1 rows: 9 coarse rows)
    ("enc0_1:f", "enc0_fwd_1", FWD, "mfma", (0, 1, 8, 4, 2, 1, 0), (683, 34, 130)),
    ("enc0_2:f", "enc0_fwd_2", FWD, "mfma", (0, 2, 8, 4, 2, 1, 0), (683, 34, 130)),
    ("wres:f", "igemm_wres", FWD, "mfma", (0, 16, 32, 4, 2, 1, 0), (171, 34, 66)),
    # BP_IMPL_BF16: every layer of the table above, in either direction, that b_config marks persistent
    ("bf16_p:16_32:f", "igemm_bf16_p", FWD, "bf16", (0, 16, 32, 4, 2, 1, 0), (3, 34, 130)),
    ("bf16_pf:16_32:d", "igemm_bf16_pf", BWD, "bf16", (0, 16, 32, 4, 2, 1, 0), (171, 33, 129)),
    ("bf16_pf:T32_16:f", "igemm_bf16_pf", FWD, "bf16", (1, 32, 16, 4, 2, 1, 0), (171, 17, 65)),
    ("bf16_p:T32_16:d", "igemm_bf16_p", BWD, "bf16", (1, 32, 16, 4, 2, 1, 0), (3, 17, 65)),
    ("bf16_p:T16_8:f", "igemm_bf16_p", FWD, "bf16", (1, 16, 8, 8, 4, 2, 0), (3, 17, 65)),          # (16 phases, one launch row each)
    ("bf16_p:8_16:d", "igemm_bf16_p", BWD, "bf16", (0, 8, 16, 8, 4, 2, 0), (3, 65, 257)),
    ("bf16_p:1_8:f", "igemm_bf16_p", FWD, "bf16", (0, 1, 8, 4, 2, 1, 0), (3, 34, 130)),
    ("bf16_pf:1_8:d", "igemm_bf16_pf", BWD, "bf16", (0, 1, 8, 4, 2, 1, 0), (171, 33, 129)),
    ("bf16_p:2_8:f", "igemm_bf16_p", FWD, "bf16", (0, 2, 8, 4, 2, 1, 0), (3, 34, 130)),
    ("bf16_pf:2_8:d", "igemm_bf16_pf", BWD, "bf16", (0, 2, 8, 4, 2, 1, 0), (171, 33, 129)),
]
ENTRIES = [Entry(t, i, d, impl, tuple(conv) + tuple(nhw)) for t, i, d, impl, conv, nhw in _TABLE]

# Cases at which this sweep found the library wrong: (tag, inst, direction, impl, case, what was wrong).  Each stays.
REGRESSIONS = []
ENTRIES += [Entry("regression:" + t, i, d, impl, tuple(c)) for t, i, d, impl, c, _ in REGRESSIONS]

# The layers of the table (a layer and its data gradient name two of the kernels): searched for persistent bf16 forms
LAYERS = sorted({e.case[:7] for e in ENTRIES if e.impl == "mfma"})


def case_id(e):
    return "%s-%dx%dx%d" % ((e.tag,) + tuple(e.case[7:]))


# ---------------------------------------------------------------------------------------------------------------------
# Host arithmetic, restated from the launch code the records cite.
def _cdiv(a, b):
    return -(-a // b)


def geom(case, direction):
    """ConvGeom of common.hpp (bp_geom_forward / bp_geom_backward_data) as a dict."""
    tr, ci, co, k, s, p = case[:6]
    gathered, produced = S.gathered_produced(case, direction)
    transposed_gather = bool(tr) != (direction == BWD)
    g = dict(T=transposed_gather, k=k, stride=s, pad=p, cin=gathered, cout=produced)
    if transposed_gather:
        g.update(nphase=s, taps=_cdiv(k, s), IS=1, OS=s)
    else:
        g.update(nphase=1, taps=k, IS=s, OS=1)
    return g


def operand_shapes(case, direction):
    """((n, c, h, w) of the gathered tensor, of the produced tensor)."""
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    x, y = (n, ci, h, w), (n, co, ho, wo)
    return (x, y) if direction == FWD else (y, x)


def tiles(e):
    """(tiles per image along y, along x) of the produced tensor."""
    r = INST[e.inst]
    _, (n, c, h, w) = operand_shapes(e.case, e.direction)
    phase = geom(e.case, e.direction)["OS"] if r.kid is None else r.phase          # (the bf16 kernel: any stride)
    return _cdiv(_cdiv(h, phase), r.th), _cdiv(_cdiv(w, phase), r.tw)


def channel_blocks(e):
    """grid.z of the igemm kernels: blocks of produced channels (16 NT WN each)."""
    g = geom(e.case, e.direction)
    if e.inst == "igemm_wres":
        return _cdiv(g["cout"], 16 * (2 if g["cout"] > 16 else 1))
    c = bf16_config(g)
    return c["cout_padP"] // c["COB"]


def plan(e, n=None):
    """(tiles, workgroups, fewest tiles of a workgroup, most) of the launch at batch n (default: the case's own)."""
    r = INST[e.inst]
    ty, tx = tiles(e)
    nt = ty * tx * (e.case[7] if n is None else n)
    if r.walk == "stride":
        grid = min(nt, r.cap)
        return nt, grid, nt // grid, _cdiv(nt, grid)
    gz = channel_blocks(e)
    if e.inst == "igemm_wres":
        nb = max(min(r.cap // gz, nt), 1)
    elif e.inst == "igemm_bf16_p":                       # (one launch row per phase: phases share the 512)
        nb = max(512 // (gz * geom(e.case, e.direction)["nphase"] ** 2), 64)
    else:
        nb = 512 // gz
    per = max(_cdiv(nt, nb), r.min_per)
    grid = _cdiv(nt, per)
    return nt, grid, nt - (grid - 1) * per, per


def walks(e):
    """The tile sequence of every workgroup (per produced-channel block and launch row), in the order it walks them."""
    nt, grid, lo, hi = plan(e)
    if INST[e.inst].walk == "stride":
        return [list(range(b, nt, grid)) for b in range(grid)]
    return [list(range(b * hi, min(nt, (b + 1) * hi))) for b in range(grid)]


def smallest_n(e):
    """The smallest batch at which every workgroup walks at least three tiles and some walk more."""
    for n in range(1, 4096):
        nt, grid, lo, hi = plan(e, n)
        if lo >= 3 and hi > lo:
            return n
    raise AssertionError(e.tag)


def _round_up(a, b):
    return _cdiv(a, b) * b


def _t_i0(p, pad, stride, taps):
    return (p + pad) // stride - (taps - 1)


def bf16_config(g):
    """b_config of conv_bf16.hpp for a layer with at most 64 produced channels (four waves): the fields the sweep needs,
    or None where the layer has no bf16 kernel."""
    nT = _cdiv(g["cout"], 16)
    assert nT <= 4, "restated for the four-wave candidates only"
    cand = ((4, 2), (4, 1), (2, 2), (2, 1), (1, 2), (1, 1))
    first = 1 if nT >= 3 else (3 if nT == 2 else 5)
    for i in range(first, 6):
        if 16 * cand[i][0] * cand[i][1] > 16 * nT and i != first:
            continue
        c = _bf16_config_for(g, *cand[i])
        if c and c["ok"]:
            return c
    return None


def _bf16_config_for(g, NT, WN):
    cin, IS, taps = g["cin"], g["IS"], g["taps"]
    CC = 32 if cin % 32 == 0 else (cin if cin in (16, 8) else (4 if cin <= 4 else 0))
    if not CC:
        return None
    R, nchunk = 32 // CC, (cin // 32 if CC == 32 else 1)
    COB = 16 * NT * WN
    nrun = rmax = 0
    for xm in range(min(IS, taps)):
        nr = _cdiv(_cdiv(taps - xm, IS), R)
        nrun += nr
        rmax = max(rmax, nr * R)
    if nrun > 16:
        return None
    TM = (4 // WN) * 4
    BH = TM // 2
    IH, IWq = (BH - 1) * IS + taps, 32 + rmax - 1
    U = min(CC, 8)

    def in_bytes(ih, iwq):
        return ((_round_up(ih * IS * iwq, 16) * CC + 511) & ~511) * 2

    def slots(ih, iwq):
        return _cdiv(ih * IS * iwq * (CC // U), 256)

    lds = in_bytes(IH, IWq) + 2 * nrun * COB * 32 * 2 + 3 * nchunk * CC * 4
    ok = lds <= 80 * 1024 and slots(IH, IWq) <= 12
    RED = 4 * 128 * 2 * 8
    lds_p = in_bytes(IH, IWq) + taps * nrun * COB * 32 * 2 + RED
    persistent = ok and NT <= 2 and nchunk == 1 and lds_p <= 64 * 1024 and (IS == 2 or g["nphase"] > 1)
    fuse = False
    if persistent and g["T"] and g["nphase"] == 2:
        spread = _t_i0(g["nphase"] - 1, g["pad"], g["stride"], taps) - _t_i0(0, g["pad"], g["stride"], taps)
        lds_f = in_bytes(IH + spread, IWq + spread) + 4 * taps * nrun * COB * 32 * 2 + RED
        fuse = lds_f <= 64 * 1024 and slots(IH + spread, IWq + spread) <= 12
    return dict(ok=ok, persistent=persistent, fuse=fuse, NT=NT, WN=WN, COB=COB, BH=BH, cout_padP=_round_up(g["cout"], COB))


def bf16_inst(case, direction):
    """The record of the persistent bf16 kernel that serves a layer, or None."""
    c = bf16_config(geom(case, direction))
    if not c or not c["persistent"]:
        return None
    return "igemm_bf16_pf" if c["fuse"] else "igemm_bf16_p"


# ---------------------------------------------------------------------------------------------------------------------
# Operands of the exact pass: small integers drawn per element, so that a pixel taken from the wrong tile or image
# changes the result, and every product and partial sum is an integer or half-integer that fp32 adds exactly in any order.
EXACT_LIMIT = float(1 << 24)            # in half-units
MAX_X, MAX_W, MAX_BIAS = 2, 1, 3


def exact_inputs(e, index):
    """(gathered tensor NCHW, w in torch's layout, bias or None, pending activation or None), float32.
    gathered tensor in -2 .. 2, w in -1 .. 1; forward: scale 1, shift in {0, 1} (1 on the first channel: act(0) != 0, a
    halo that skipped the mask shows), slope in {0, 1/2, 1}, and an integer bias on every other case."""
    rng = np.random.Generator(np.random.PCG64([47, index]))
    gshape, pshape = operand_shapes(e.case, e.direction)
    g = rng.integers(-MAX_X, MAX_X + 1, size=gshape).astype(np.float32)
    w = rng.integers(-MAX_W, MAX_W + 1, size=S.weight_shape(e.case)).astype(np.float32)
    if e.direction == BWD:
        return g, w, None, None
    ci, co = e.case[1], e.case[2]
    shift = rng.integers(0, 2, size=ci).astype(np.float32)
    shift[0] = 1.0
    slope = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=ci)
    bias = rng.integers(-MAX_BIAS, MAX_BIAS + 1, size=co).astype(np.float32) if index % 2 == 0 else None
    return g, w, bias, (np.ones(ci, np.float32), shift, slope)


def exact_magnitude(e):
    """An upper bound, in half-units, of the sum of |products| (+ |bias|) behind any element of the exact pass: what no
    partial sum in any order can pass."""
    k = e.case[3]
    gathered, _ = S.gathered_produced(e.case, e.direction)
    act = MAX_X + 1 if e.direction == FWD else MAX_X                # |act(x)| <= |x| + shift
    return 2.0 * (k * k * gathered * act * MAX_W + MAX_BIAS)


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference of one direction (torch on the CPU; conv_sweep.reference computes all four quantities of a case in
# numpy, which these tensors are too large for).  test_walk_sweep_host.py pins it to conv_sweep.reference.
def _conv(case, direction, ga, w, bias):
    tr, ci, co, k, s, p, op, n, h, wd = case
    F = torch.nn.functional
    ga, w = torch.from_numpy(np.ascontiguousarray(ga, np.float64)), torch.from_numpy(np.ascontiguousarray(w, np.float64))
    if direction == FWD:
        y = F.conv_transpose2d(ga, w, stride=s, padding=p, output_padding=op) if tr else F.conv2d(ga, w, stride=s, padding=p)
        if bias is not None:
            y = y + torch.from_numpy(np.asarray(bias, np.float64))[None, :, None, None]
        return y.numpy()
    if tr:
        return F.conv2d(ga, w, stride=s, padding=p)[:, :, :h, :wd].contiguous().numpy()
    ho, wo = S.out_shape(case)
    rest = (h - ((ho - 1) * s - 2 * p + k), wd - ((wo - 1) * s - 2 * p + k))       # trailing rows no output reads
    return F.conv_transpose2d(ga, w, stride=s, padding=p, output_padding=rest).numpy()


def reference(case, direction, g, w, bias, pw, round_act=None):
    """float64 y = conv(act(x)) [+ bias] (forward) or dx = d / d act(x) of the gathered dy (data gradient)."""
    return _conv(case, direction, S.activated(g, pw, round_act), w, bias)


def bound(case, direction, g, w, bias, pw, round_act=None):
    """The same of the operands' magnitudes: the sum of |product| behind every element (+ |bias|)."""
    return _conv(case, direction, np.abs(S.activated(g, pw, round_act)), np.abs(np.asarray(w, np.float64)),
                 None if bias is None else np.abs(bias))


def terms(case, direction):
    """Number of products behind every element, (1, 1, h, w): the same in every image and produced channel."""
    tr, ci, co, k, s, p, op, n, h, w = case
    one = (tr, 1, 1, k, s, p, op, 1, h, w)
    gshape, _ = operand_shapes(one, direction)
    gathered, _ = S.gathered_produced(case, direction)
    return _conv(one, direction, np.ones(gshape), np.ones((1, 1, k, k)), None) * gathered
