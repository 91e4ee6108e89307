"""Weight-gradient cases at which a split walks several tiles, their integer test data and its float64 reference
(plain module, no test in here).

Every weight-gradient kernel of csrc/ has nsplit = min(units, cap) workgroups, each walking the tiles split,
split + nsplit, ... of dy and writing one partial image; conv_sweep.py draws tensors so small that nsplit == units and
no tile loop sees a second iteration.  INST below is one record per kernel instantiation the C ABI can reach -- the
extent of dy per unit (read from the kernel: the file and constant are named per record), the cap, and how the kernel
brings the next tile in -- and pick() derives from it the smallest (n, h, w) with n >= 2 and h, w no multiples of the
tile that sits in a regime:

  A   cap < units < 2 cap (so units % nsplit != 0): two iterations, some splits one tile short
  B   units >= 2 cap + 1, units % cap != 0: three iterations, the pipeline in steady state
  C   units == cap exactly
  R   the one-channel kernel (no cap: one split per 256 pixel quads): nsplit 64 and 65 -- the two shapes of the
      reduction -- and 100 (1e6 pixels: what the exact range of the integer data admits)
  F   the kernels that fold their own partial rows 32 at a time: a grid of 33 rows (two chunks); the grid at its cap is C
  W   the output-stationary trunk kernels (no cap: splits = n x bands x strips): two extents with different band heights

test_wgrad_sweep_host.py pins all of this to bp_conv_backward_weight_plan without a GPU; test_gpu_wgrad_sweep.py runs the
cases.  The data are small integers (x in -2..2, dy in -1..1, pending activation with scales 1 and 2, shifts +-1, slopes
1/2, 1/4 and 0), so that every product and partial sum is a multiple of 1/4 below 2^24 quarter-units and dW, dbias are
exact in fp32 and bf16 in any order of summation: one pixel dropped or counted twice shows as a difference of at least 1/4.
"""
import collections

import torch

import conv_sweep as S

MAX_TENSOR_BYTES = 64 << 20            # x and dy of every case, in fp32
EXACT_LIMIT = float(1 << 24)           # quarter-units: every sum must stay below this

# ---------------------------------------------------------------------------------------------------------------------
# The instantiations.  cap: ("target", T, CXC, CYC, KHB): ceil(T / (ceil(cx / CXC) ceil(cy / CYC) ceil(k / KHB)));
# ("general", T): the same with 16-channel X tiles, 16 or 32-channel Y blocks and one tap row per workgroup;
# ("fixed", N); ("quads",): one split per 256 units; ("bands",): no cap.
Inst = collections.namedtuple("Inst", "family tw th cap style where")
INST = {}


def _wt(name, khb, kw, s, ntx, nty, wx, wy, wk, bh, dma=False):
    """conv_wgrad_tiles.hip BP_WT(KHB, KW, S, NTX, NTY, WX, WY, WK, BH[, DMA]): tile 16 x BH (tiles_x = ceil(w / 16))."""
    INST[name] = Inst("tiles_dma" if dma else "tiles", 16, bh, ("target", 512, 16 * ntx * wx, 16 * nty * wy, khb),
                      "LDS-DMA into the other buffer, one tile ahead" if dma else "staged through registers, no prefetch",
                      "conv_wgrad_tiles.hip BP_WT(%d, %d, %d, %d, %d, %d, %d, %d, %d%s)"
                      % (khb, kw, s, ntx, nty, wx, wy, wk, bh, ", true" if dma else ""))


_wt("wt_k3s1_64x64_dma", 3, 3, 1, 2, 2, 2, 2, 1, 3, True)
_wt("wt_k3s1_64x64", 3, 3, 1, 2, 2, 2, 2, 1, 4)
_wt("wt_k3s1_16x32", 3, 3, 1, 1, 2, 1, 1, 4, 8)
_wt("wt_k3s1_16x16", 3, 3, 1, 1, 1, 1, 1, 4, 8)
_wt("wt_k4s2_32x64_dma", 4, 4, 2, 1, 2, 2, 2, 1, 2, True)
_wt("wt_k4s2_32x64", 4, 4, 2, 1, 2, 2, 2, 1, 4)
_wt("wt_k4s2_16x32_dma", 4, 4, 2, 1, 2, 1, 1, 4, 4, True)
_wt("wt_k4s2_16x32", 4, 4, 2, 1, 2, 1, 1, 4, 4)
_wt("wt_k4s2_16x16", 4, 4, 2, 1, 1, 1, 1, 4, 4)
_wt("wt_k3s2_32x64_dma", 3, 3, 2, 1, 2, 2, 2, 1, 2, True)
_wt("wt_k3s2_32x64", 3, 3, 2, 1, 2, 2, 2, 1, 4)
_wt("wt_k3s2_16x32", 3, 3, 2, 1, 2, 1, 1, 4, 4)
_wt("wt_k3s2_16x16", 3, 3, 2, 1, 1, 1, 1, 4, 4)
_wt("wt_k4s1_32x64_dma", 4, 4, 1, 1, 2, 2, 2, 1, 4, True)
_wt("wt_k4s1_32x64", 4, 4, 1, 1, 2, 2, 2, 1, 4)
_wt("wt_k4s1_16x32", 4, 4, 1, 1, 2, 1, 1, 4, 8)
_wt("wt_k4s1_16x16", 4, 4, 1, 1, 1, 1, 1, 4, 8)
_wt("wt_k9s1", 3, 9, 1, 1, 1, 1, 1, 4, 8)
_wt("wt_k5s1", 5, 5, 1, 1, 1, 1, 1, 4, 8)
_wt("wt_k7s1", 4, 7, 1, 1, 1, 1, 1, 4, 8)
_wt("wt_k8s4", 4, 8, 4, 1, 1, 1, 1, 4, 2)


def _ws(k, s, cxs, cys, bh):
    """conv_wgrad_small.hip BP_WS(K, S, CXS, CYS, BH): tile 32 x BH, cap 1024; the next tile's loads are issued before
    the k-steps of the current one (PIPE) unless the kernel holds more than 16 accumulator tiles."""
    tpm, tpn = 16 // cxs, 16 // cys
    gx, gy = -(-k // tpm), s * -(-(-(-k // s)) // tpn)
    name = "ws_k%ds%d_%dx%d" % (k, s, cxs, cys)
    INST[name] = Inst("small", 32, bh, ("fixed", 1024),
                      "next tile in registers behind the k-steps" if gy * gx <= 16 else "load and commit back to back",
                      "conv_wgrad_small.hip BP_WS(%d, %d, %d, %d, %d)" % (k, s, cxs, cys, bh))
    return name


for _a in ((7, 1, 16, 8, 8), (5, 1, 4, 16, 8), (5, 1, 16, 8, 8), (3, 1, 16, 8, 8), (3, 1, 8, 16, 8), (3, 1, 4, 16, 8),
           (3, 1, 8, 8, 8), (5, 1, 8, 8, 8), (7, 1, 1, 1, 16), (9, 1, 2, 16, 8), (9, 1, 1, 16, 8), (9, 1, 16, 1, 8),
           (9, 1, 16, 2, 4), (4, 2, 1, 8, 8), (4, 2, 2, 8, 8), (4, 2, 1, 1, 16), (8, 4, 8, 16, 2), (8, 4, 1, 1, 8)):
    _ws(*_a)
# BP_WS lines no call reaches without an environment switch: conv_wgrad_thin.hip takes their layers first
UNREACHABLE = {
    "BP_WS(5, 1, 8, 1, 16)": "5 ... 8 -> 1 k5 is thin_cy1's layer",
    "BP_WS(3, 1, 1, 1, 16)": "1 -> 1 k3 is thin_c1's layer (up to 65535 splits: 6.7e7 pixels)",
    "BP_WS(5, 1, 1, 1, 16)": "1 -> 1 k5 is thin_c1's layer",
}
for _n in ("ws_k9s1_16x1", "ws_k9s1_16x2", "ws_k9s1_1x16", "ws_k9s1_2x16"):
    INST["chunk_" + _n[3:]] = INST[_n]._replace(family="small_chunked", where=INST[_n].where + " per 16-channel chunk (conv_wgrad.hip chunked_run)")


def _wb(name, khb, kw, s, ntx, nty, wx, wy, bh, wt=False):
    """conv_wgrad_bf16.hip BP_WB_(KHB, KW, S, NTX, NTY, WX, WY, BH[, WT]): tile 32 x BH."""
    INST[name] = Inst("bf16_tiled", 32, bh, ("target", 512, 16 * ntx * wx, 16 * nty * wy, khb),
                      "next tile fetched into registers while this one multiplies",
                      "conv_wgrad_bf16.hip BP_WB_(%d, %d, %d, %d, %d, %d, %d, %d%s)" % (khb, kw, s, ntx, nty, wx, wy, bh, ", true" if wt else ""))


_wb("wb_k3s1_64x64", 3, 3, 1, 2, 2, 2, 2, 4)
_wb("wb_k3s1_32x32", 3, 3, 1, 2, 2, 1, 1, 8)
_wb("wb_k3s1_16x32", 3, 3, 1, 1, 2, 1, 1, 8)
_wb("wb_k3s1_32x16", 3, 3, 1, 2, 1, 1, 1, 8)
_wb("wb_k3s1_16x16", 3, 3, 1, 1, 1, 1, 1, 8)
_wb("wb_k4s2_64x64", 2, 4, 2, 2, 2, 2, 2, 2)
_wb("wb_k4s2_32x64_wt", 4, 4, 2, 2, 4, 1, 1, 4, True)
_wb("wb_k4s2_32x32", 2, 4, 2, 2, 2, 1, 1, 4)
_wb("wb_k4s2_16x32_wt", 4, 4, 2, 1, 2, 1, 1, 8, True)
_wb("wb_k4s2_16x32", 4, 4, 2, 1, 2, 1, 1, 4)
_wb("wb_k4s2_32x16", 4, 4, 2, 2, 1, 1, 1, 4)
_wb("wb_k4s2_16x16", 4, 4, 2, 1, 1, 1, 1, 4)
_wb("wb_k5s1", 5, 5, 1, 1, 1, 1, 1, 8)
_wb("wb_k7s1", 4, 7, 1, 1, 1, 1, 1, 8)

INST.update({
    "general": Inst("general", 16, 8, ("general", 2048), "staged through LDS, no prefetch", "conv_wgrad.hip WG_BW x WG_BH, wgrad_general"),
    "enc": Inst("enc", 16, 2, ("fixed", 768), "persistent over tiles", "conv_enc.hip wgrad_enc: 16 x EW_R, cap 768"),
    "thin_cy1": Inst("thin_cy1", 32, 16, ("fixed", 1280), "next tile's loads issued before the k-steps",
                     "conv_wgrad_thin.hip launch_cy1<5, 8, 16>: Cy1Cfg::BW x BH, cap 1280"),
    "thin_c1": Inst("thin_c1", 4, 16, ("quads",), "one pass, 256 quads of 4 pixels x C1_BR rows per split",
                    "conv_wgrad_thin.hip launch_c1: qpr = ceil(w / 4), nbands = ceil(h / C1_BR)"),
    "stem": Inst("stem", 64, 8, ("fixed", 1024), "persistent; folds its rows 32 at a time", "conv_stem.hip TW x TH, stem_wgrad_grid"),
    "flat": Inst("flat", 32, 8, ("fixed", 512), "persistent; folds its rows 32 at a time", "conv_wgrad_flat.hip TW x TH, flat_grid"),
    "flat_s2": Inst("flat_s2", 32, 4, ("fixed", 512), "next tile in registers; folds its rows 32 at a time",
                    "conv_wgrad_flat.hip s2::SW x s2::SH, s2::grid_of"),
    "ws_f32": Inst("ws_f32", 0, 0, ("bands",), "output-stationary, one band of rows per split", "conv_wgrad_ws_f32.hip ww_bands"),
    "ws_bf16": Inst("ws_bf16", 0, 0, ("bands",), "output-stationary, one band of rows per split", "conv_wgrad_ws_bf16.hip wo_bands"),
    "bf16_wf": Inst("bf16_wf", 64, 16, ("fixed", 512), "persistent, next tile in registers", "conv_wgrad_bf16.hip WF_TW x WF_TH, wgrad_wf"),
    "bf16_sf": Inst("bf16_sf", 64, 16, ("fixed", 512), "persistent, next tile in registers", "conv_wgrad_bf16.hip SF_TW x SF_TH, wgrad_sf"),
    "bf16_wh": Inst("bf16_wh", 64, 16, ("fixed", 1024), "persistent, next tile in registers", "conv_wgrad_bf16.hip WH_TW x WH_TH, wgrad_wh"),
})
SHARED_TARGET = 448                    # conv_wgrad_tiles.hip shared_target: tap-blocked fp32 launches below 1.5e11 flop
SHARED_FLAT_GRID = 256                 # conv_wgrad_flat.hip shared_grid: one workgroup per CU (256 without a device, too)
# What a view with odd channel stride and offset falls to (a record not named here serves both kinds of view)
ODD = {"wt_k3s1_64x64_dma": "wt_k3s1_64x64", "wt_k4s2_32x64_dma": "wt_k4s2_32x64", "wt_k4s2_16x32_dma": "wt_k4s2_16x32",
       "wt_k3s2_32x64_dma": "wt_k3s2_32x64", "wt_k4s1_32x64_dma": "wt_k4s1_32x64", "flat": "ws_k7s1_16x8",
       "flat_s2": "wt_k4s2_16x32", "ws_f32": "wt_k3s1_64x64"}
ALIGNED = {v: k for k, v in ODD.items() if k.startswith("wt_")}
SELF_REDUCING = ("stem", "flat", "flat_s2")
DEFERRING = ("ws_f32", "enc", "thin_c1", "thin_cy1", "small", "tiles", "tiles_dma", "general")
BF16_FAMILIES = ("bf16_tiled", "bf16_wf", "bf16_sf", "bf16_wh", "ws_bf16")


# ---------------------------------------------------------------------------------------------------------------------
def xy_channels(case):
    """(X, Y) channel counts: X is the tensor on the fine grid, Y the one whose tiles are walked."""
    return (case[2], case[1]) if case[0] else (case[1], case[2])


def y_extent(case):
    """(n, h, w) of Y: dy for a convolution, the module input for a transposed one."""
    n, h, w = case[7:]
    return (n, h, w) if case[0] else (n,) + S.out_shape(case)


def units(inst, case):
    n, yh, yw = y_extent(case)
    r = INST[inst]
    if r.cap[0] == "bands":
        return None
    return n * -(-yw // r.tw) * -(-yh // r.th)


def cap(inst, case, shared=False):
    r = INST[inst]
    cx, cy = xy_channels(case)
    k = case[3]
    if r.cap[0] == "fixed":
        return min(r.cap[1], SHARED_FLAT_GRID) if shared and r.family in ("flat", "flat_s2") else r.cap[1]
    if r.cap[0] == "target":
        _, target, cxc, cyc, khb = r.cap
        n, yh, yw = y_extent(case)
        if shared and r.family in ("tiles", "tiles_dma") and 2.0 * n * yh * yw * k * k * cx * cy < 1.5e11:
            target = SHARED_TARGET
        base = -(-cx // cxc) * -(-cy // cyc) * -(-k // khb)
        return -(-target // base)
    if r.cap[0] == "general":
        base = -(-cx // 16) * -(-cy // (32 if cy > 16 else 16)) * k
        return -(-r.cap[1] // base)
    return None


def _bands(n, h, strips):
    br = h
    while br > 8 and n * strips * -(-h // br) < 64:
        br = -(-br // 2)
    return br, -(-h // br)


def band_rows(inst, case):
    n, h, w = case[7:]
    return _bands(n, h, (w // 64 if w > 64 else 1) if inst == "ws_f32" else 1)[0]


def nsplit(inst, case, shared=False):
    """Partial images the library writes for the case: min(units, cap) of the table."""
    r = INST[inst]
    if r.cap[0] == "quads":
        return -(-units(inst, case) // 256)
    if r.cap[0] == "bands":
        n, h, w = case[7:]
        strips = (w // 64 if w > 64 else 1) if inst == "ws_f32" else 1
        return n * strips * _bands(n, h, strips)[1]
    return min(units(inst, case), cap(inst, case, shared))


def in_regime(inst, case, regime):
    u, c = units(inst, case), cap(inst, case)
    if regime == "A":
        return c < u < 2 * c and u % c != 0
    if regime == "B":
        return u >= 2 * c + 1 and u % c != 0
    if regime == "C":
        return u == c
    if regime == "F":
        return 33 <= u <= 64 and u < c
    if regime[0] == "R":
        return -(-u // 256) == int(regime[1:]) and u % 256 != 0
    if regime[0] == "W":
        return band_rows(inst, case) == int(regime[1:])
    raise ValueError(regime)


def _module_extent(conv, y):
    """Module input extent that gives Y the extent y."""
    tr, _, _, k, s, p, _ = conv
    return y if tr else (y - 1) * s + k - 2 * p


def pick(inst, conv, regime):
    """The (n, h, w), n >= 2, with the fewest pixels of Y at which `inst` is in `regime`: Y has tx x ty tiles per image,
    its width three short (at least one short) of tx tiles and its height one short of ty tiles, at least two of each."""
    r = INST[inst]
    c = cap(inst, tuple(conv) + (2, _module_extent(conv, 2 * r.th - 1), _module_extent(conv, 2 * r.tw - 1)))
    if regime[0] == "R":
        want = [256 * (int(regime[1:]) - 1) + 1]
    else:
        want = {"A": [c + 1], "B": [2 * c + 1], "C": [c], "F": [33]}[regime]
    best = None
    for n in range(2, 9):
        for tx in range(2, 17):
            ty = max(2, -(-want[0] // (n * tx)))
            yw, yh = tx * r.tw - min(3, r.tw - 1), ty * r.th - 1
            case = tuple(conv) + (n, _module_extent(conv, yh), _module_extent(conv, yw))
            if S.valid(case) and y_extent(case) == (n, yh, yw) and in_regime(inst, case, regime):
                key = (n * yh * yw, n, tx)
                if best is None or key < best[0]:
                    best = (key, case)
    if best is None:
        raise ValueError("no extent puts %s in regime %s" % (inst, regime))
    return best[1]


def tensor_bytes(case):
    """Bytes of the larger of x and dy in fp32."""
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    return 4 * max(n * h * w * ci, n * ho * wo * co)


def layout(c, kind, bf16=False):
    """(cstride, coff) of a view of c channels inside a wider buffer: a 16-byte addressable slice, or one with odd
    stride and offset."""
    if kind == "aligned":
        q = 8 if bf16 else 4
        return (c + q - 1) // q * q + q, q
    cs = c + 3
    return cs + (cs % 2 == 0), 1


# ---------------------------------------------------------------------------------------------------------------------
# The layers: (record the regime is reached in, kind of view it is reached through, (transposed, cin, cout, k, stride,
# pad, out_pad), regimes, impl the record belongs to, element types of (x, dy)).
#                                                   every BP_WT line: the DMA ones aligned, their plain twins odd
LAYERS = [
    ("wt_k3s1_64x64_dma", "aligned", (0, 20, 24, 3, 1, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k3s1_64x64", "odd", (0, 20, 24, 3, 1, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k3s1_16x32", "aligned", (0, 8, 24, 3, 1, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k3s1_16x16", "aligned", (0, 16, 16, 3, 1, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s2_32x64_dma", "aligned", (0, 20, 36, 4, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s2_32x64", "odd", (0, 20, 36, 4, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s2_16x32_dma", "aligned", (0, 8, 24, 4, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s2_16x32", "odd", (0, 8, 24, 4, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s2_16x16", "aligned", (0, 8, 8, 4, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k3s2_32x64_dma", "aligned", (0, 20, 36, 3, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k3s2_32x64", "odd", (0, 20, 36, 3, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k3s2_16x32", "aligned", (0, 8, 24, 3, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k3s2_16x16", "aligned", (0, 8, 8, 3, 2, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s1_32x64_dma", "aligned", (0, 20, 36, 4, 1, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s1_32x64", "odd", (0, 20, 36, 4, 1, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s1_16x32", "aligned", (0, 8, 24, 4, 1, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k4s1_16x16", "aligned", (0, 8, 8, 4, 1, 1, 0), "ABC", "mfma", "ff"),
    ("wt_k9s1", "aligned", (0, 8, 8, 9, 1, 4, 0), "ABC", "mfma", "ff"),
    ("wt_k5s1", "aligned", (0, 16, 16, 5, 1, 2, 0), "ABC", "mfma", "ff"),
    ("wt_k7s1", "aligned", (0, 8, 8, 7, 1, 3, 0), "ABC", "mfma", "ff"),
    ("wt_k8s4", "aligned", (0, 4, 8, 8, 4, 2, 0), "ABC", "mfma", "ff"),
    # every reachable BP_WS line
    ("ws_k7s1_16x8", "aligned", (0, 12, 8, 7, 1, 3, 0), "ABC", "mfma", "ff"),
    ("ws_k5s1_4x16", "aligned", (0, 4, 16, 5, 1, 2, 0), "ABC", "mfma", "ff"),
    ("ws_k5s1_16x8", "aligned", (0, 16, 8, 5, 1, 2, 0), "ABC", "mfma", "ff"),
    ("ws_k3s1_16x8", "aligned", (0, 16, 8, 3, 1, 1, 0), "ABC", "mfma", "ff"),
    ("ws_k3s1_8x16", "aligned", (0, 8, 16, 3, 1, 1, 0), "ABC", "mfma", "ff"),
    ("ws_k3s1_4x16", "aligned", (0, 3, 16, 3, 1, 1, 0), "ABC", "mfma", "ff"),
    ("ws_k3s1_8x8", "aligned", (0, 7, 8, 3, 1, 1, 0), "ABC", "mfma", "ff"),
    ("ws_k5s1_8x8", "aligned", (0, 8, 5, 5, 1, 2, 0), "ABC", "mfma", "ff"),
    ("ws_k7s1_1x1", "aligned", (0, 1, 1, 7, 1, 3, 0), "ABC", "mfma", "ff"),
    ("ws_k9s1_2x16", "aligned", (0, 2, 16, 9, 1, 4, 0), "ABC", "mfma", "ff"),
    ("ws_k9s1_1x16", "aligned", (0, 1, 12, 9, 1, 4, 0), "ABC", "mfma", "ff"),
    ("ws_k9s1_16x1", "aligned", (0, 16, 1, 9, 1, 4, 0), "ABC", "mfma", "ff"),
    ("ws_k9s1_16x2", "aligned", (0, 10, 2, 9, 1, 4, 0), "ABC", "mfma", "ff"),
    ("ws_k4s2_1x8", "aligned", (0, 1, 8, 4, 2, 1, 0), "ABC", "mfma", "ff"),
    ("ws_k4s2_2x8", "aligned", (0, 2, 8, 4, 2, 1, 0), "ABC", "mfma", "ff"),
    ("ws_k4s2_1x1", "aligned", (0, 1, 1, 4, 2, 1, 0), "ABC", "mfma", "ff"),
    ("ws_k8s4_8x16", "aligned", (0, 8, 16, 8, 4, 3, 0), "ABC", "mfma", "ff"),
    ("ws_k8s4_1x1", "aligned", (0, 1, 1, 8, 4, 2, 0), "ABC", "mfma", "ff"),
    # the chunked k9 wrapper, a ragged last chunk (28 = 16 + 12) on either side
    ("chunk_k9s1_16x1", "aligned", (0, 28, 1, 9, 1, 4, 0), "AC", "mfma", "ff"),
    ("chunk_k9s1_16x2", "aligned", (0, 28, 2, 9, 1, 4, 0), "AC", "mfma", "ff"),
    ("chunk_k9s1_1x16", "aligned", (0, 1, 28, 9, 1, 4, 0), "AC", "mfma", "ff"),
    ("chunk_k9s1_2x16", "aligned", (1, 28, 2, 9, 1, 4, 0), "AC", "mfma", "ff"),
    # the one-channel tails
    ("thin_cy1", "aligned", (0, 8, 1, 5, 1, 2, 0), "ABC", "mfma", "ff"),
    ("thin_cy1", "aligned", (0, 5, 1, 5, 1, 2, 0), "A", "mfma", "ff"),
    ("thin_c1", "aligned", (0, 1, 1, 3, 1, 1, 0), ("R64", "R65", "R100"), "mfma", "ff"),
    ("thin_c1", "aligned", (0, 1, 1, 5, 1, 2, 0), ("R64", "R65", "R100"), "mfma", "ff"),
    # the k8 stride-4 layer in both orientations
    ("enc", "aligned", (0, 8, 16, 8, 4, 2, 0), "ABC", "mfma", "ff"),
    ("enc", "aligned", (1, 16, 8, 8, 4, 2, 0), "A", "mfma", "ff"),
    # the general kernel: k6 s1 with one Y tile, k2 s3 with two (the transposed layer of conv_sweep.REGRESSIONS)
    ("general", "aligned", (0, 3, 16, 6, 1, 2, 0), "ABC", "mfma", "ff"),
    ("general", "aligned", (1, 24, 33, 2, 3, 0, 1), "ABC", "mfma", "ff"),
    # the kernels that reduce themselves
    ("stem", "aligned", (0, 3, 16, 5, 1, 2, 0), "ABCF", "mfma", "ff"),
    ("flat", "aligned", (0, 16, 8, 7, 1, 3, 0), "ABCF", "mfma", "ff"),
    ("flat_s2", "aligned", (0, 16, 32, 4, 2, 1, 0), "ABCF", "mfma", "ff"),
    ("flat_s2", "aligned", (1, 32, 16, 4, 2, 1, 0), "ACF", "mfma", "ff"),
    # the bf16 tiled variants, by the operand types they take
    ("wb_k3s1_64x64", "aligned", (0, 36, 40, 3, 1, 1, 0), "ABC", "bf16", "bb"),
    ("wb_k3s1_32x32", "aligned", (0, 20, 24, 3, 1, 1, 0), "ABC", "bf16", "bb"),
    ("wb_k3s1_16x32", "aligned", (0, 8, 24, 3, 1, 1, 0), "ABC", "bf16", "ff"),
    ("wb_k3s1_32x16", "aligned", (0, 24, 8, 3, 1, 1, 0), "ABC", "bf16", "bb"),
    ("wb_k3s1_16x16", "aligned", (0, 8, 8, 3, 1, 1, 0), "ABC", "bf16", "bf"),
    ("wb_k4s2_64x64", "aligned", (0, 36, 40, 4, 2, 1, 0), "ABC", "bf16", "bb"),
    ("wb_k4s2_32x64_wt", "aligned", (0, 20, 36, 4, 2, 1, 0), "ABC", "bf16", "bb"),
    ("wb_k4s2_32x32", "aligned", (0, 20, 24, 4, 2, 1, 0), "ABC", "bf16", "ff"),
    ("wb_k4s2_16x32_wt", "aligned", (0, 8, 24, 4, 2, 1, 0), "ABC", "bf16", "bb"),
    ("wb_k4s2_16x32", "aligned", (0, 8, 36, 4, 2, 1, 0), "ABC", "bf16", "fb"),
    ("wb_k4s2_32x16", "aligned", (1, 8, 24, 4, 2, 1, 0), "ABC", "bf16", "bb"),
    ("wb_k4s2_16x16", "aligned", (0, 8, 8, 4, 2, 1, 0), "ABC", "bf16", "bb"),
    ("wb_k5s1", "aligned", (0, 8, 8, 5, 1, 2, 0), "ABC", "bf16", "bb"),
    ("wb_k7s1", "aligned", (0, 8, 8, 7, 1, 3, 0), "ABC", "bf16", "ff"),
    # the bf16 flattened kernels: wf wants x in bf16, sf x in fp32 and dy in bf16, wh x in bf16 and dy in fp32
    ("bf16_wf", "aligned", (0, 16, 8, 7, 1, 3, 0), "ABC", "bf16", "bb"),
    ("bf16_sf", "aligned", (0, 3, 16, 5, 1, 2, 0), "ABC", "bf16", "fb"),
    ("bf16_wh", "aligned", (0, 8, 1, 5, 1, 2, 0), "ABC", "bf16", "bf"),
]
# The output-stationary trunk kernels at two band heights (extents typed in: their widths are the kernels' gate)
TRUNK = (0, 128, 128, 3, 1, 1, 0)
FIXED = [
    ("ws_f32", "aligned", TRUNK + (2, 20, 32), "W5", "mfma", "ff"),
    ("ws_f32", "aligned", TRUNK + (2, 64, 32), "W8", "mfma", "ff"),
    ("ws_bf16", "aligned", TRUNK + (2, 20, 32), "W5", "bf16", "bb"),
    ("ws_bf16", "aligned", TRUNK + (2, 64, 32), "W8", "bf16", "bb"),
]
# Regime B where x or dy would pass MAX_TENSOR_BYTES, or the sums of the integer data 2^24 quarter-units: (record, conv)
DROPPED_B = {
    ("general", (1, 24, 33, 2, 3, 0, 1)): "685 tiles of 16 x 8 at stride 3: dy of 90 MB",
    ("bf16_wh", (0, 8, 1, 5, 1, 2, 0)): "2049 tiles of 64 x 16: 2e6 terms per element, 1.6 times the exact range",
}

Entry = collections.namedtuple("Entry", "tag inst kind regime case impl dt")


def _entries():
    out = []
    for inst, kind, conv, regimes, impl, dt in LAYERS:
        for regime in regimes:
            if regime == "B" and (inst, conv) in DROPPED_B:
                continue
            case = pick(inst, conv, regime)
            tag = "%s:%s:%s%d_%d_k%d" % (inst, regime, "T" if conv[0] else "C", conv[1], conv[2], conv[3])
            out.append(Entry(tag, inst, kind, regime, case, impl, dt))
    for inst, kind, case, regime, impl, dt in FIXED:
        out.append(Entry("%s:%s" % (inst, regime), inst, kind, regime, case, impl, dt))
    assert len({e.tag for e in out}) == len(out)
    return out


ENTRIES = _entries()
# Cases at which this sweep once found the library wrong: (tag, case, what was wrong) -- beyond conv_sweep.MAX_*, so
# kept here and not in conv_sweep.REGRESSIONS
REGRESSIONS = []


def pairs():
    """Every (family, regime) the module promises."""
    return sorted({(INST[e.inst].family, e.regime) for e in ENTRIES})


def expected_inst(entry, kind):
    """The record a view of `kind` is served by (fp32 operands)."""
    if kind == entry.kind:
        return entry.inst
    return ODD.get(entry.inst, entry.inst) if kind == "odd" else ALIGNED.get(entry.inst, entry.inst)


def case_id(e):
    return "%s-%dx%dx%d" % ((e.tag,) + tuple(e.case[7:]))


# ---------------------------------------------------------------------------------------------------------------------
# Integer data.  A counter-based generator in 31-bit arithmetic (no product passes 2^57): the same draws from numpy-free
# torch on any device and version.
def draws(count, seed, mod, device="cpu"):
    i = torch.arange(count, dtype=torch.int64, device=device)
    v = (i * 1103515245 + 12345 + (seed % 1000003) * 2654435) & 0x7FFFFFFF
    v = ((v ^ (v >> 15)) * 1664525 + 1013904223) & 0x7FFFFFFF
    v = ((v ^ (v >> 13)) * 22695477 + 1) & 0x7FFFFFFF
    return ((v ^ (v >> 16)) >> 4) % mod


def int_pointwise(case, index):
    """Pending activation of the module input: scale 1 or 2, shift +-1 (act(0) != 0: padding is zero AFTER the
    activation), slope 1/2, 1/4 or 0 -- float32 tensors of cin."""
    ci = case[1]
    c = torch.arange(ci)
    scale = torch.tensor([1.0, 2.0])[(c + index) % 2]
    slope = torch.tensor([0.5, 0.25, 0.0])[c % 3]
    shift = torch.where(slope == 0, torch.tensor(1.0), torch.tensor([1.0, -1.0])[(c // 2 + index) % 2])      # (ReLU channels: + 1)
    return scale, shift, slope


def int_inputs(case, index, device="cpu"):
    """(x, dy, (scale, shift, slope)): NHWC float32 tensors, x in -2..2 and dy in -1..1."""
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    x = (draws(n * h * w * ci, 2 * index + 1, 5, device) - 2).to(torch.float32).reshape(n, h, w, ci)
    dy = (draws(n * ho * wo * co, 2 * index + 2, 3, device) - 1).to(torch.float32).reshape(n, ho, wo, co)
    return x, dy, int_pointwise(case, index)


def activated(x, pw, round_bf16=False):
    """float64 act(x) of an NHWC tensor as the kernels stage it (conv_sweep.activated): t = fma(x, scale, shift) rounded
    once to float32, then the leaky ReLU in float64 -- or, for the bf16 kernels, in float32 and rounded to bf16."""
    scale, shift, slope = (v.to(x.device) for v in pw)
    t = (x.double() * scale.double() + shift.double()).float()
    if round_bf16:
        return torch.where(t > 0, t, t * slope).to(torch.bfloat16).double()
    t = t.double()
    return torch.where(t > 0, t, t * slope.double())


def reference_dw(case, xa, dy):
    """float64 dW in torch's layout from the ACTIVATED module input xa and dy (NHWC float64 tensors), one matrix product
    per tap:  dW[cy][cx][ky][kx] = sum_{n,q} X[n, q s + k - p, cx] Y[n, q, cy]."""
    tr, ci, co, k, s, p, op, n, h, w = case
    X, Y = (dy, xa) if tr else (xa, dy)
    _, yh, yw, cy = Y.shape
    _, xh, xw, cx = X.shape
    ph, pw_ = max((yh - 1) * s + k - p, xh) - xh, max((yw - 1) * s + k - p, xw) - xw
    Xp = torch.zeros((n, p + xh + ph, p + xw + pw_, cx), dtype=torch.float64, device=X.device)
    Xp[:, p:p + xh, p:p + xw] = X
    # (the pixels in chunks of 2048, one batched product and a sum over the chunks: a single product of two thin
    #  matrices a million pixels long is the slowest shape a GEMM library has)
    P, CH = n * yh * yw, 2048
    B = -(-P // CH)
    rows = lambda t, c: torch.nn.functional.pad(t.reshape(P, c), (0, 0, 0, B * CH - P)).reshape(B, CH, c)
    Yb = rows(Y, cy).transpose(1, 2).contiguous()
    out = torch.empty((cy, cx, k, k), dtype=torch.float64, device=X.device)
    for ky in range(k):
        for kx in range(k):
            Xs = Xp[:, ky:ky + (yh - 1) * s + 1:s, kx:kx + (yw - 1) * s + 1:s]
            out[:, :, ky, kx] = torch.bmm(Yb, rows(Xs, cx)).sum(dim=0)
    return out


def terms_dw(case, device="cpu"):
    """Products behind each tap of dW (any channel pair): the reference of all-ones single-channel operands."""
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    one = (tr, 1, 1, k, s, p, op, n, h, w)
    return reference_dw(one, torch.ones((n, h, w, 1), dtype=torch.float64, device=device),
                        torch.ones((n, ho, wo, 1), dtype=torch.float64, device=device))


def max_activation(pw):
    """max |act(x)| over x in -2..2 and the channels."""
    scale, shift, slope = (v.double() for v in pw)
    return float(torch.maximum(2 * scale + shift, (2 * scale - shift) * slope).max())


def magnitude_bound(dy, pw):
    """An upper bound, in quarter-units, of the sum of |products| behind any element of dW or dbias and so of every
    partial sum a kernel can form: max |act(x)| x the largest per-channel sum of |dy| (each dy element meets at most
    one x element per tap, whichever operand is on the fine grid)."""
    per_channel = dy.abs().double().sum(dim=(0, 1, 2)).max()
    return 4.0 * max(max_activation(pw), 1.0) * float(per_channel)
