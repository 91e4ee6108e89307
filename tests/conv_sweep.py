"""Convolution geometries for the dispatcher sweep, and their float64 reference (plain module, no test in here).

The convolution entry points of include/bp_hip.h take any bp_conv on any valid view; three host-side heuristics
(igemm_config / bp_igemm_run, b_config, bp_wgrad_select) pick a kernel and its tiling from the geometry alone.  cases()
lists small tensors at many geometries, in two strata:

  grid      every k in 1..9, stride in 1..4, pad in {0, (k-1)//2, k//2, k-1, k+1}, both forms and, for the transposed
            form, every out_pad < stride: 504 cells, channels and extents drawn per cell from a fixed generator;
  targeted  the layers that the special kernels are gated on (bp_*_ok), each with the same layer one field away, so that
            both sides of every gate run, plus hand-picked cases for the paths the model's own layers never reach.

test_conv_sweep_ref.py pins reference() to torch in float64 and measures which kernels the dispatcher picks for the
cases; test_gpu_conv_sweep.py runs every implementation on them.
"""
import numpy as np

from oracle import ops

CHANNELS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 24, 31, 32, 33, 48, 64, 65, 80, 96, 128, 130)
KS, STRIDES = range(1, 10), range(1, 5)
MAX_N, MAX_H, MAX_W = 3, 22, 40
MAX_OUT_H, MAX_OUT_W = 34, 52           # the produced side of a transposed layer stays near the gathered side's limits
MAX_MACS = 2.5e8                        # multiply-adds of one forward: keeps the float64 reference of the sweep cheap
SEED = 1


def pads_of(k):
    return sorted({0, (k - 1) // 2, k // 2, k - 1, k + 1})


def grid_cells():
    """(transposed, k, stride, pad, out_pad) of every cell, in a fixed order."""
    cells = []
    for k in KS:
        for s in STRIDES:
            for p in pads_of(k):
                cells.append((0, k, s, p, 0))
                cells.extend((1, k, s, p, op) for op in range(s))
    return cells


def out_extent(case_or_conv, n_in):
    """Module output extent along one axis (torch's formula); <= 0: no such layer."""
    tr, _, _, k, s, p, op = case_or_conv[:7]
    if tr:
        return (n_in - 1) * s - 2 * p + k + op
    return (n_in + 2 * p - k) // s + 1 if n_in + 2 * p - k >= 0 else 0


def out_shape(case):
    return out_extent(case, case[8]), out_extent(case, case[9])


def valid(case):
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = out_shape(case)
    return (ci > 0 and co > 0 and k > 0 and s > 0 and p >= 0 and 0 <= op < s + (s == 1) and (tr or op == 0)
            and n > 0 and h > 0 and w > 0 and ho > 0 and wo > 0)


class _Lcg:
    """64-bit linear congruential generator (Knuth's MMIX constants): the same draws on every machine and version."""

    def __init__(self, seed):
        self.s = (seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
        for _ in range(4):
            self.below(2)

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.s >> 33) % n


def _macs(case):
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = out_shape(case)
    return float(k * k * ci * co * n) * (h * w if tr else ho * wo)


def _draw_cell(cell, index):
    """Channels and extents of one grid cell.  A draw without positive output extents, with a produced side beyond
    MAX_OUT_* or with more arithmetic than MAX_MACS is drawn again (the cell is never dropped); after 200 draws the
    extents are the smallest valid ones."""
    tr, k, s, p, op = cell
    g = _Lcg(SEED * 1000003 + index)
    ci, co = CHANNELS[g.below(len(CHANNELS))], CHANNELS[g.below(len(CHANNELS))]
    for _ in range(200):
        n, h, w = 1 + g.below(MAX_N), 1 + g.below(MAX_H), 1 + g.below(MAX_W)
        case = (tr, ci, co, k, s, p, op, n, h, w)
        ho, wo = out_shape(case)
        if valid(case) and ho <= MAX_OUT_H and wo <= MAX_OUT_W and _macs(case) <= MAX_MACS:
            return case
    hmin = next(h for h in range(1, 64) if out_extent((tr, ci, co, k, s, p, op), h) > 0)
    return (tr, ci, co, k, s, p, op, 1, hmin, hmin + 1)


def grid_cases():
    return [_draw_cell(cell, i) for i, cell in enumerate(grid_cells())]


# ---------------------------------------------------------------------------------------------------------------------
# Targeted stratum.  A gate is the layer a special kernel is built for: (name, module layer, family of the kernel id of
# (forward, data gradient) -- see family() -- and the one-field changes that stay INSIDE the gate in that direction).
# Every other change listed in NEIGHBOUR_FIELDS must leave the gate: test_conv_sweep_ref.py checks both claims against
# bp_conv_kernel_id, so a loosened bp_*_ok shows up there before it shows up as a wrong number.
#                 (transposed, cin, cout, k, stride, pad, out_pad)
GATES = [
    # conv_stem.hip: 3 -> 16 k5, flattened (tap column, channel) K
    ("stem", (0, 3, 16, 5, 1, 2, 0), ("700000", None), ((), ())),
    # conv_flat.hip flat_kernel: unit-stride k7 that gathers 8 and produces 16 channels (forward)
    ("flat_k7_8_16", (0, 8, 16, 7, 1, 3, 0), ("710000", "750000"), ((), ())),
    # ... the head's first layer 16 -> 8 k7: forward flat_h7 (K split over two waves), data gradient flat_kernel
    ("flat_h7_16_8", (0, 16, 8, 7, 1, 3, 0), ("750000", "710000"), ((), ())),
    # conv_flat.hip stride-2 k4 gather 32 -> 64 (forward); its data gradient is the four-phase 64 -> 32 kernel
    ("flat_g4_32_64", (0, 32, 64, 4, 2, 1, 0), ("730000", "740000"), ((), ())),
    # ... the same two kernels with the roles swapped
    ("flat_t64_64_32", (1, 64, 32, 4, 2, 1, 0), ("740000", "730000"), (("out_pad+1",), ("out_pad+1",))),
    # conv_flat.hip four-phase transposed form 32 -> 16 k4 s2 (forward)
    ("flat_t4_32_16", (1, 32, 16, 4, 2, 1, 0), ("720000", None), (("out_pad+1",), ())),
    # ... as the data gradient of the conv layer 16 -> 32 (whose forward is the weights-resident igemm)
    ("wres_16_32", (0, 16, 32, 4, 2, 1, 0), ("wres", "720000"), (("cout-1", "pad+1", "pad-1", "k+1", "k-1"), ())),
    # conv_enc.hip: k8 stride-4 8 -> 16 forward and data gradient
    ("enc_8_16", (0, 8, 16, 8, 4, 2, 0), ("760000", "770000"), ((), ())),
    ("enc_t_16_8", (1, 16, 8, 8, 4, 2, 0), ("770000", "760000"), (("out_pad+1",), ("out_pad+1",))),
    # conv_enc.hip enc0: k4 s2 {1, 2} -> 8 at the full-resolution end of the recognition / prior networks
    ("enc0_1_8", (0, 1, 8, 4, 2, 1, 0), ("780001", None), ((), ())),
    ("enc0_2_8", (0, 2, 8, 4, 2, 1, 0), ("780002", None), ((), ())),
    # conv_small.hip tiny kernels: one channel on both sides, k4 s2 and k8 s4, both forms (the pad is free)
    ("tiny_k4", (1, 1, 1, 4, 2, 1, 0), ("tiny", "tiny"), (("pad+1", "pad-1", "out_pad+1"),) * 2),
    ("tiny_k8", (1, 1, 1, 8, 4, 2, 0), ("tiny", "tiny"), (("pad+1", "pad-1", "out_pad+1"),) * 2),
    # conv_small.hip vector-ALU kernels: the heads' 8 -> 1 k5 tail (the pad is free) ...
    ("small_8_1_k5", (0, 8, 1, 5, 1, 2, 0), ("small", "small"), (("pad+1", "pad-1", "k-1"), ("pad+1", "pad-1"))),
    # ... the CGAN's k9 head 32 -> 1 (any multiple of 8 up to 64 into one or two channels)
    ("small_32_1_k9", (0, 32, 1, 9, 1, 4, 0), ("small", None), (("pad+1", "pad-1", "cout+1"), ())),
    # ... and the PatchGAN logits k4 (multiples of 8 into one channel)
    ("small_64_1_k4", (0, 64, 1, 4, 1, 1, 0), ("small", None), (("pad+1", "pad-1"), ())),
    # the 128 -> 128 k3 trunk layer: eight-wave LDS-DMA igemm (and, by views, the weights-stationary kernel)
    ("trunk_128", (0, 128, 128, 3, 1, 1, 0), ("dma8", "dma8"),
     (("pad+1", "pad-1", "k+1", "k-1", "cout-1", "cout+1"), ("pad+1", "pad-1", "k+1", "k-1", "cin-1", "cin+1", "stride"))),
]
NEIGHBOUR_FIELDS = ("pad+1", "pad-1", "k+1", "k-1", "cin+1", "cin-1", "cout+1", "cout-1", "stride", "out_pad+1")
_FIELD_INDEX = {"cin": 1, "cout": 2, "k": 3, "pad": 5, "out_pad": 6}


def neighbour(conv, field):
    """The layer `conv` with one field changed (None where that is no valid layer): stride toggles 2 <-> 1 (4 -> 2)."""
    c = list(conv)
    if field == "stride":
        c[4] = {1: 2, 2: 1, 4: 2}.get(c[4], 1)
        c[6] = min(c[6], c[4] - 1)
    else:
        name, delta = field[:-2], 1 if field[-2] == "+" else -1
        c[_FIELD_INDEX[name]] += delta
    tr, ci, co, k, s, p, op = c
    if ci < 1 or co < 1 or k < 1 or p < 0 or op < 0 or op >= s or (op and not tr):
        return None
    return tuple(c)


def _extents(conv, n, h, w):
    """`conv` on (n, h, w), grown until the output is positive."""
    while out_extent(conv, h) <= 0:
        h += 1
    while out_extent(conv, w) <= 0:
        w += 1
    return tuple(conv) + (n, h, w)


def gate_cases():
    """[(tag, case)]: every gate at two sizes (less than one tile; ragged across several) and its neighbours."""
    out = []
    for name, conv, _, _ in GATES:
        tr, s = conv[0], conv[4]
        big = (3, 9, 13) if tr and s == 4 else ((3, 15, 23) if tr else (3, 22, 40))
        out.append(("gate:" + name, _extents(conv, 2, 5, 7)))
        out.append(("gate:" + name + ":ragged", _extents(conv, *big)))
        for f in NEIGHBOUR_FIELDS:
            nb = neighbour(conv, f)
            if nb is not None:
                out.append(("near:%s:%s" % (name, f), _extents(nb, 2, 6 if tr else 11, 9 if tr else 19)))
    return out


# Hand-picked cases for the gaps the model's layers leave (numbers: the list in the module docstring of
# test_gpu_conv_sweep.py).          (transposed, cin, cout, k, stride, pad, out_pad, n, h, w)
EXTRA = [
    # 1. wide layers whose unaligned views drop from the LDS-DMA kernels to the plain igemm_kernel <16,4,2,*>, <16,4,1,*>,
    #    <16,2,1,*>, <8,*,*,*>
    ("wide:128_130_k3", (0, 128, 130, 3, 1, 1, 0, 2, 9, 21)),
    ("wide:64_48_k3", (0, 64, 48, 3, 1, 1, 0, 2, 11, 18)),
    ("wide:48_32_k5", (0, 48, 32, 5, 1, 2, 0, 2, 8, 20)),
    ("wide:24_96_k3", (0, 24, 96, 3, 1, 1, 0, 3, 7, 17)),
    ("wide:8_80_k3s2", (0, 8, 80, 3, 2, 1, 0, 2, 12, 25)),
    ("wide:T96_24_k4s2", (1, 96, 24, 4, 2, 1, 0, 2, 6, 11)),
    # 2. channel counts off the grid: zero-padded chunk tails (cin % 16 = 1, % 8 = 1, % 4 = 1), cc_first 8 and 4
    ("chan:17_16_k3", (0, 17, 16, 3, 1, 1, 0, 2, 9, 17)),
    ("chan:9_33_k3", (0, 9, 33, 3, 1, 1, 0, 2, 9, 17)),
    ("chan:5_17_k3", (0, 5, 17, 3, 1, 1, 0, 2, 9, 17)),
    ("chan:33_65_k3", (0, 33, 65, 3, 1, 1, 0, 2, 9, 17)),
    ("chan:T31_7_k3s2", (1, 31, 7, 3, 2, 1, 1, 2, 7, 9)),
    #    ... the `co < cout` mask of every channel-block shape: cout = 16 m + 1, 16 m - 1
    ("chan:16_31_k3", (0, 16, 31, 3, 1, 1, 0, 2, 9, 17)),
    ("chan:32_49_k3", (0, 32, 49, 3, 1, 1, 0, 2, 9, 17)),
    ("chan:32_81_k3", (0, 32, 81, 3, 1, 1, 0, 2, 9, 17)),
    #    ... pixel packing with COP 4 and 8 (cout in 3 .. 8 with cin <= 16), next to COP 1 and 2
    ("cop:16_3_k3", (0, 16, 3, 3, 1, 1, 0, 2, 9, 37)),
    ("cop:12_4_k5", (0, 12, 4, 5, 1, 2, 0, 2, 9, 37)),
    ("cop:4_5_k3", (0, 4, 5, 3, 1, 1, 0, 2, 9, 37)),
    ("cop:7_8_k5", (0, 7, 8, 5, 1, 2, 0, 2, 9, 37)),
    ("cop:16_7_k1", (0, 16, 7, 1, 1, 0, 0, 2, 9, 37)),
    ("cop:9_2_k3", (0, 9, 2, 3, 1, 1, 0, 2, 9, 37)),
    ("cop:12_1_k7", (0, 12, 1, 7, 1, 3, 0, 2, 9, 37)),
    ("cop:T3_6_k3", (1, 3, 6, 3, 1, 1, 0, 2, 9, 37)),
    #    ... and just past its limit (cin 17: not packed)
    ("cop:17_4_k3", (0, 17, 4, 3, 1, 1, 0, 2, 9, 37)),
    # 3. transposed-form tap masks: k % stride != 0, k < stride (phases without a tap: exactly the bias), stride 3
    ("taps:T_k1s2", (1, 8, 16, 1, 2, 0, 1, 2, 7, 9)),
    ("taps:T_k2s3", (1, 16, 16, 2, 3, 0, 2, 2, 7, 9)),
    ("taps:T_k1s4", (1, 4, 32, 1, 4, 0, 3, 2, 5, 6)),
    ("taps:T_k5s3", (1, 16, 32, 5, 3, 2, 1, 2, 7, 9)),
    ("taps:T_k6s4", (1, 32, 16, 6, 4, 1, 0, 2, 5, 7)),
    ("taps:T_k2s1", (1, 16, 16, 2, 1, 0, 0, 2, 7, 9)),
    ("taps:C_k1s3", (0, 16, 32, 1, 3, 0, 0, 2, 11, 17)),       # data gradient: input pixels no output reads
    ("taps:C_k2s4", (0, 32, 16, 2, 4, 0, 0, 2, 13, 19)),
    ("taps:C_k6s1", (0, 16, 16, 6, 1, 2, 0, 2, 11, 17)),
    # 4. padding and extents: pad 0, pad >= k, trailing rows no output reads, h = 1, w = 1, output 1 x 1
    ("ext:pad0_k5", (0, 16, 32, 5, 1, 0, 0, 2, 9, 17)),
    ("ext:pad6_k5", (0, 16, 32, 5, 1, 6, 0, 2, 3, 4)),
    ("ext:trailing_s3", (0, 16, 32, 3, 3, 0, 0, 2, 11, 17)),    # (11 - 3) % 3 = 2 trailing rows, (17 - 3) % 3 = 2 columns
    ("ext:trailing_s2", (0, 32, 64, 4, 2, 1, 0, 2, 11, 17)),    # ... through the conv_flat.hip pair
    ("ext:h1", (0, 16, 32, 3, 1, 1, 0, 3, 1, 40)),
    ("ext:w1", (0, 16, 32, 3, 1, 1, 0, 3, 22, 1)),
    ("ext:out1x1", (0, 32, 32, 4, 2, 0, 0, 3, 4, 4)),
    ("ext:in1x1_T", (1, 32, 32, 4, 2, 1, 0, 3, 1, 1)),
    ("ext:in1x1_k7", (0, 16, 8, 7, 1, 3, 0, 1, 1, 1)),          # the head's gate on a single pixel
    ("ext:T_outpad_s4", (1, 16, 16, 8, 4, 2, 3, 2, 3, 5)),
    ("ext:T_pad_ge_k", (1, 16, 16, 3, 2, 4, 1, 2, 9, 11)),
    # the weights-resident igemm: cin 16 with a stride-2 gather or >= 5 taps, one or two 16-channel blocks
    ("wres:16_16_k3s2", (0, 16, 16, 3, 2, 1, 0, 2, 13, 21)),
    ("wres:16_24_k5", (0, 16, 24, 5, 1, 2, 0, 2, 9, 17)),
    ("wres:16_32_k6", (0, 16, 32, 6, 1, 3, 0, 2, 9, 17)),
    ("wres:T24_16_k4s2", (1, 24, 16, 4, 2, 1, 0, 2, 6, 9)),     # (as the data gradient: gathers 16)
    # widths the weights-stationary kernels take (bp_set_option switches them against the tiled kernels)
    ("ws:128_128_k3_w32", (0, 128, 128, 3, 1, 1, 0, 2, 9, 32)),
    ("ws:64_128_k4s2_w32", (0, 64, 128, 4, 2, 1, 0, 2, 16, 32)),
    ("ws:T128_64_k4s2_w16", (1, 128, 64, 4, 2, 1, 0, 2, 7, 16)),
    # the stem's gate on one row and on one column
    ("stem:h1", (0, 3, 16, 5, 1, 2, 0, 3, 1, 40)),
    ("stem:w1", (0, 3, 16, 5, 1, 2, 0, 2, 22, 1)),
    # the vector-ALU kernels at their other instantiations
    ("small:1_8_k5", (0, 1, 8, 5, 1, 2, 0, 2, 9, 37)),
    ("small:16_1_k5", (0, 16, 1, 5, 1, 0, 0, 2, 9, 37)),
    ("small:1_1_k3", (0, 1, 1, 3, 1, 1, 0, 2, 9, 37)),
    ("small:2_64_k9", (0, 2, 64, 9, 1, 4, 0, 1, 9, 21)),        # (its data gradient: 64 -> 2 k9)
    ("small:T1_1_k3", (1, 1, 1, 3, 1, 0, 0, 2, 9, 37)),
    ("tiny:C1_1_k4s2", (0, 1, 1, 4, 2, 0, 0, 2, 9, 37)),
    ("tiny:C1_1_k8s4", (0, 1, 1, 8, 4, 3, 0, 2, 9, 37)),
]

# bp_conv_kernel_id of (forward, data gradient) of every EXTRA case: what keeps each comment above honest -- a "wide"
# case must sit on an LDS-DMA id (1xxxxx / 2xxxxx / 3xxxxx: the same CC, NT, WN, MT digits name the plain kernel its odd
# view falls to), a "chan" case on the chunk width its comment names, a "wres" / "small" / "tiny" case in that family.
# test_conv_sweep_ref.py compares; a retuned heuristic that moves a case shows there and the case is re-picked.
EXTRA_IDS = {
    "wide:128_130_k3": (216424, 16424),
    "wide:64_48_k3": (116414, 116414),
    "wide:48_32_k5": (316214, 108414),
    "wide:24_96_k3": (208424, 316214),
    "wide:8_80_k3s2": (108424, 316114),
    "wide:T96_24_k4s2": (316214, 108424),
    "chan:17_16_k3": (16114, 316214),
    "chan:9_33_k3": (8414, 16114),
    "chan:5_17_k3": (8214, 16114),
    "chan:33_65_k3": (16424, 16414),
    "chan:T31_7_k3s2": (16114, 8214),
    "chan:16_31_k3": (316214, 16114),
    "chan:32_49_k3": (116414, 16214),
    "chan:32_81_k3": (216424, 16214),
    "cop:16_3_k3": (8114, 4114),
    "cop:12_4_k5": (8114, 4114),
    "cop:4_5_k3": (4114, 8114),
    "cop:7_8_k5": (8114, 8114),
    "cop:16_7_k1": (16114, 8114),
    "cop:9_2_k3": (4114, 4114),
    "cop:12_1_k7": (4111, 4114),
    "cop:T3_6_k3": (4114, 8114),
    "cop:17_4_k3": (16114, 4214),
    "taps:T_k1s2": (8114, 416112),
    "taps:T_k2s3": (316114, 4114),
    "taps:T_k1s4": (4214, 4114),
    "taps:T_k5s3": (316214, 4114),
    "taps:T_k6s4": (316114, 8211),
    "taps:T_k2s1": (316114, 316114),
    "taps:C_k1s3": (4214, 316114),
    "taps:C_k2s4": (4114, 316214),
    "taps:C_k6s1": (416112, 416112),
    "ext:pad0_k5": (416212, 316114),
    "ext:pad6_k5": (416212, 316114),
    "ext:trailing_s3": (4214, 316114),
    "ext:trailing_s2": (730000, 740000),
    "ext:h1": (316214, 316114),
    "ext:w1": (316214, 316114),
    "ext:out1x1": (8214, 316214),
    "ext:in1x1_T": (316214, 8214),
    "ext:in1x1_k7": (750000, 710000),
    "ext:T_outpad_s4": (316114, 8111),
    "ext:T_pad_ge_k": (316114, 416112),
    "wres:16_16_k3s2": (416112, 316114),
    "wres:16_24_k5": (416212, 16114),
    "wres:16_32_k6": (416222, 316114),
    "wres:T24_16_k4s2": (16114, 416212),
    "ws:128_128_k3_w32": (216424, 216424),
    "ws:64_128_k4s2_w32": (108424, 116414),
    "ws:T128_64_k4s2_w16": (116414, 108424),
    "stem:h1": (700000, 8114),
    "stem:w1": (700000, 8114),
    "small:1_8_k5": (905018, 905081),
    "small:16_1_k5": (905161, 4114),
    "small:1_1_k3": (903011, 903011),
    "small:2_64_k9": (4414, 909642),
    "small:T1_1_k3": (903011, 903011),
    "tiny:C1_1_k4s2": (842110, 842111),
    "tiny:C1_1_k8s4": (884110, 884111),
}

# Cases that once gave a wrong answer: (tag, case, what was wrong).  Each one stays in the sweep for good.
REGRESSIONS = [
    # the general weight-gradient kernel (conv_wgrad.hip wgrad_kernel, every (k, stride) without a tap-blocked or
    # tap-packed variant: here k6) reduced its partial sums with the row length of dW left at 0: every produced channel
    # landed on the first one's row and the rest of dW was never written
    ("wgrad_general_k6", (0, 3, 16, 6, 1, 2, 0, 2, 11, 19), "dW of the general kernel: only dW[0] written"),
    # the chunked k9 weight gradient (one or two channels against a wide side, 16 channels at a time) was entered when a
    # FULL chunk had an instantiation: with 33 = 2 x 16 + 1 channels the last chunk had none, and the call returned
    # BP_EUNSUPPORTED -- also under BP_IMPL_AUTO -- after the first two chunks of dW had been written
    ("wgrad_chunked_k9_ragged", (0, 33, 1, 9, 1, 4, 0, 2, 11, 19), "refusal after partial writes; AUTO refused"),
    ("wgrad_chunked_k9_ragged_y", (0, 2, 35, 9, 1, 4, 0, 2, 11, 19), "the same with the wide side produced"),
    # bf16 forward of a stride-2 transposed layer with few gathered and more than 32 produced channels: b_config marked
    # it persistent + phase-fused, but only blocks of <= 32 channels have that kernel, and the tiled kernel ran on the
    # fused tile geometry (max error 0.7 ... 1.0 of the tensor's maximum with out_pad = 1)
    ("bf16_fused_geometry_wide_block", (1, 16, 130, 2, 2, 1, 1, 3, 6, 21), "bf16 forward wrong: 0.709 of max |y|"),
    ("bf16_fused_geometry_k3", (1, 3, 48, 3, 2, 1, 1, 3, 8, 11), "bf16 forward wrong: 1.0 of max |y|"),
    ("wgrad_general_k2s3_two_blocks", (1, 24, 40, 2, 3, 0, 1, 2, 5, 7), "the same with two 16-channel Y tiles per workgroup"),
]


def tagged_cases():
    """[(tag, case)]: the whole sweep in a fixed order; tags are unique and spell the stratum."""
    out = [("grid:%03d" % i, c) for i, c in enumerate(grid_cases())]
    out += gate_cases() + list(EXTRA) + [("regression:" + t, c) for t, c, _ in REGRESSIONS]
    return out


def cases():
    return [c for _, c in tagged_cases()]


def case_id(tag, case):
    tr, ci, co, k, s, p, op, n, h, w = case
    return "%s-%s%d_%d_k%ds%dp%d%s-%dx%dx%d" % (tag, "T" if tr else "C", ci, co, k, s, p, "o%d" % op if op else "", n, h, w)


def checksum(cs):
    """Order-dependent 64-bit sum of a case list (FNV-1a over the fields)."""
    hsh = 0xCBF29CE484222325
    for c in cs:
        for v in c:
            hsh = ((hsh ^ (int(v) & 0xFFFFFFFF)) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return hsh


# ---------------------------------------------------------------------------------------------------------------------
def family(kid):
    """Kernel family of a bp_conv_kernel_id."""
    if kid < 0:
        return "none"
    if kid >= 900000:
        return "small"
    if kid >= 800000:
        return "tiny"
    if kid >= 700000:
        return str(kid)
    if kid >= 100000:
        return {1: "dma4", 2: "dma8", 3: "dmaf", 4: "wres"}[kid // 100000]
    return "plain-mt%d" % (kid % 10)


def igemm_shape(kid):
    """(CC, NT, WN) of an igemm id (any of the plain / dma / dmaf / wres families), else None."""
    if kid < 0 or kid >= 700000:
        return None
    r = kid % 100000
    return r // 1000, (r // 100) % 10, 1 if kid >= 400000 else (r // 10) % 10


def gathered_produced(case, direction):
    """(gathered, produced) channel counts of the forward (0) / data gradient (1)."""
    return (case[1], case[2]) if direction == 0 else (case[2], case[1])


# ---------------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """float32 -> nearest bfloat16 (ties to even), returned as float32.  Finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def weight_shape(case):
    tr, ci, co, k = case[:4]
    return ((ci, co) if tr else (co, ci)) + (k, k)


def make_inputs(case, index, with_bias):
    """Seeded float32 operands: x, w (torch layout), bias or None, dy, and a pending activation (scale, shift, slope)
    with act(0) != 0 (padding is zero AFTER the activation) and a few ReLU channels."""
    tr, ci, co, k, s, p, op, n, h, w = case
    rng = np.random.Generator(np.random.PCG64([41, index]))
    ho, wo = out_shape(case)
    x = rng.standard_normal((n, ci, h, w)).astype(np.float32)
    wt = (rng.standard_normal(weight_shape(case)) * 0.2).astype(np.float32)
    bias = rng.standard_normal(co).astype(np.float32) if with_bias else None
    dy = rng.standard_normal((n, co, ho, wo)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, ci).astype(np.float32)
    shift = rng.uniform(0.2, 0.6, ci).astype(np.float32)
    slope = rng.uniform(0.05, 0.3, ci).astype(np.float32)
    slope[2::3] = 0.0
    return x, wt, bias, dy, (scale, shift, slope)


def activated(x, pw, round_act=None):
    """float64 act(x) as the kernels stage it: t = fma(x, scale, shift) rounded once to float32, then the leaky
    ReLU in float64 -- or, for the bf16 kernels (`round_act`), in float32 and rounded to bf16."""
    if pw is None:
        a = np.asarray(x, np.float32)
        return (round_act(a) if round_act else a).astype(np.float64)
    scale, shift, slope = (np.asarray(v, np.float32)[None, :, None, None] for v in pw)
    t = (np.asarray(x, np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
    if round_act:
        return round_act(np.where(t > 0, t, t * slope).astype(np.float32)).astype(np.float64)
    t = t.astype(np.float64)
    return np.where(t > 0, t, t * slope.astype(np.float64))


def _conv4(case, xa, w, bias, dy):
    """(y, dx, dw, dbias) of float64 operands: xa is the ACTIVATED input."""
    tr, ci, co, k, s, p, op, n, h, wd = case
    if tr:
        y = ops.convT2d_fwd(xa, w, s, p, op)
        dx = ops.convT2d_bwd_data(dy, w, s, p)[:, :, :h, :wd]
        dw = ops.convT2d_bwd_weight(xa, dy, s, p, k, k)
    else:
        y = ops.conv2d_fwd(xa, w, s, p)
        dx = ops.conv2d_bwd_data(dy, w, s, p, h, wd)
        dw = ops.conv2d_bwd_weight(xa, dy, s, p, k, k)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[None, :, None, None]
    return y, dx, dw, dy.sum(axis=(0, 2, 3))


def reference(case, x, w, bias, dy, pw, round_act=None):
    """float64 y = conv(act(x)) [+ bias], dx = d/d act(x), dw, dbias from oracle.ops."""
    return _conv4(case, activated(x, pw, round_act), np.asarray(w, np.float64), bias, np.asarray(dy, np.float64))


def bound(case, x, w, bias, dy, pw, round_act=None):
    """The same four quantities of the operands' magnitudes: for every output element, the sum of |product| behind
    it (plus |bias|)."""
    ab = None if bias is None else np.abs(np.asarray(bias, np.float64))
    return _conv4(case, np.abs(activated(x, pw, round_act)), np.abs(np.asarray(w, np.float64)), ab,
                  np.abs(np.asarray(dy, np.float64)))


def terms(case):
    """Number of products behind every element of (y, dx, dw, dbias): the same four maps with every operand 1
    (one gathered channel, times the channel count)."""
    tr, ci, co, k, s, p, op, n, h, w = case
    one = (tr, 1, 1, k, s, p, op, n, h, w)
    ho, wo = out_shape(case)
    ty, tdx, tdw, tdb = _conv4(one, np.ones((n, 1, h, w)), np.ones((1, 1, k, k)), None, np.ones((n, 1, ho, wo)))
    return ty * ci, tdx * co, tdw, tdb


# ---------------------------------------------------------------------------------------------------------------------
# The statistics sweep (test_gpu_stats_sweep.py): the same pinned cases through the convolution + per-channel sums entry
# points, and STATS_EXTRA for what the sweep's small tensors cannot reach.  The epilogues write one row of partial sums
# per workgroup; bp_conv_stats_workspace is host arithmetic and tells how many: bytes / (16 C) = rows + folded rows.
STATS_DIRECT_ROWS = 2048                # csrc/conv_igemm.hip stats_fold_plan: up to here the last stage adds the rows itself


def fold_plan(rows):
    """(folded rows, rows per folded row) of stats_fold_plan: none up to STATS_DIRECT_ROWS, then one per 32 rows up to
    256 of them."""
    nfold = 0 if rows <= STATS_DIRECT_ROWS else ((rows + 31) // 32 if rows // 32 < 256 else 256)
    per = (rows + nfold - 1) // nfold if nfold else 0
    if nfold:
        nfold = (rows + per - 1) // per
    return nfold, per


def stats_rows(nbytes, channels, width=None):
    """Rows of partial sums behind a workspace of `nbytes` for `channels` produced channels (rows of `width` doubles,
    2 * channels unless given); None if no row count, or more than one (a few sizes next to 8192 rows), gives that size."""
    width = 2 * channels if width is None else width
    if nbytes <= 0 or nbytes % (8 * width):
        return None
    total = nbytes // (8 * width)
    found = [rows for rows in range(total, max(total - 257, 0), -1) if rows + fold_plan(rows)[0] == total]
    return found[0] if len(found) == 1 else None


def fold_regime(rows):
    """Which branch of stats_fold_plan a row count takes."""
    if rows <= STATS_DIRECT_ROWS:
        return "direct"
    return "fold32" if rows // 32 < 256 else "fold256"


# (tag, case).  The first field of a tag names what the case is for, the second the direction it is meant in (f: forward,
# d: data gradient) and the regime / row count test_conv_sweep_ref.py checks against bp_conv_stats_workspace:
#   rows:<dir>:<regime>   tiled kernel (tile of 8 x 32 phase-grid pixels), rows = phases x images x tiles: many images and
#                         phases, few pixels -- "direct" 2048 rows exactly, "fold32" rows % 32 != 0, "fold256" rows % 256 != 0
#   wres:f:walk           the weights-resident persistent kernel with more tiles than workgroups (two tiles each)
#   wide:<dir>:<C>        256 / 512 produced channels on at most two tiles; 1024: refused (stats_plan admits up to 512; its
#                         LDS condition refuses no power of two below that in any configuration the dispatcher picks)
#   walk:f:<family>       the register-resident kernels with more tiles than workgroups (grid-stride walk), the one-channel
#                         kernel and the activation-backward epilogue (act) past 2048 rows: the fold runs
#                                 (transposed, cin, cout, k, stride, pad, out_pad, n, h, w)
STATS_EXTRA = [
    ("rows:f:direct", (1, 4, 16, 4, 4, 0, 0, 32, 9, 33)),           # 16 phases x 32 images x 4 tiles = 2048
    ("rows:f:fold32", (1, 4, 16, 4, 4, 0, 0, 43, 3, 70)),           # 16 x 43 x 3 = 2064 = 64.5 x 32
    ("rows:f:fold256", (1, 4, 16, 4, 4, 0, 0, 171, 2, 65)),         # 16 x 171 x 3 = 8208 = 32 x 256 + 16
    ("rows:d:direct", (0, 16, 4, 4, 4, 0, 0, 32, 36, 132)),
    ("rows:d:fold32", (0, 16, 4, 4, 2, 1, 0, 57, 34, 130)),         # 4 phases x 57 x 9 = 2052 = 64 x 32 + 4
    ("rows:d:fold256", (0, 16, 4, 4, 4, 0, 0, 171, 8, 260)),
    ("wres:f:walk", (0, 16, 32, 4, 2, 1, 0, 257, 2, 34)),           # 257 x 2 tiles of 8 x 16 = 514 > 512 workgroups
    ("wide:f:256", (0, 8, 256, 3, 1, 1, 0, 1, 5, 20)),
    ("wide:f:512", (0, 4, 512, 1, 1, 0, 0, 1, 5, 20)),
    ("wide:d:256", (0, 256, 16, 3, 1, 1, 0, 1, 5, 20)),
    ("wide:d:512", (0, 512, 4, 3, 1, 1, 0, 2, 5, 20)),
    ("wide:f:1024", (0, 4, 1024, 1, 1, 0, 0, 1, 5, 20)),
    ("walk:f:stem", (0, 3, 16, 5, 1, 2, 0, 1025, 9, 5)),            # 1025 x 2 tiles of 8 x 64 > 2048 workgroups
    ("walk:f:flat_t4", (1, 32, 16, 4, 2, 1, 0, 257, 1, 17)),        # 257 x 2 phase-grid tiles of 8 x 16 > 512
    ("walk:f:flat_g4", (0, 32, 64, 4, 2, 1, 0, 129, 2, 34)),        # 129 x 2 tiles of 4 x 16 > 256
    ("walk:f:flat_t64", (1, 64, 32, 4, 2, 1, 0, 129, 1, 17)),       # 129 x 2 phase-grid tiles of 8 x 16 > 256
    ("walk:f:enc", (0, 8, 16, 8, 4, 2, 0, 257, 4, 68)),             # 257 x 2 tiles of 4 x 16 > 512
    ("walk:f:enc0", (0, 2, 8, 4, 2, 1, 0, 1025, 4, 66)),            # 1025 x 2 tiles of 8 x 32 > 2048
    ("walk:f:tiny", (1, 1, 1, 4, 2, 1, 0, 683, 9, 15)),             # 683 x 3 blocks of 256 pixels = 2049 rows
    ("walk:d:act", (0, 8, 1, 5, 1, 2, 0, 1025, 17, 5)),             # 1025 x 2 tiles of 16 x 64 = 2050 rows
]

# Cases at which the statistics sweep once found the library wrong: (tag, case, what was wrong).  Each stays in
# test_gpu_stats_sweep.py for good (kept apart from REGRESSIONS: the pinned convolution sweep does not change).
STATS_REGRESSIONS = [
    # conv_flat.hip's forward kernels 720000 / 730000 / 740000 refuse a produced view that is not 16-byte addressable, but
    # their workspace queries looked at the tile count alone: a caller that trusted the answer got BP_EUNSUPPORTED
    ("flat_t4_query_on_odd_view", (1, 32, 16, 4, 2, 1, 0, 2, 5, 7), "workspace > 0 on a view the kernel refuses"),
    ("flat_g4_query_on_odd_view", (0, 32, 64, 4, 2, 1, 0, 2, 6, 9), "the same for the stride-2 gather 32 -> 64"),
    ("flat_t64_query_on_odd_view", (1, 64, 32, 4, 2, 1, 0, 2, 5, 7), "the same for the transposed form 64 -> 32"),
    # conv_flat.hip flat_k7_kernel (710000, data gradient with sums) read raw 16 bytes at a time and refused any other raw
    # view -- which bp_conv_stats_workspace, not being told about raw, cannot know: it reads such a view with scalar loads now
    ("flat_k7_raw_view_not_16_byte", (0, 16, 8, 7, 1, 3, 0, 2, 5, 7), "BP_EUNSUPPORTED after a non-zero query"),
    # bp_conv_stats_workspace answers for the generic bf16 kernel as well where the weights-stationary one runs; the call
    # checked the latter's smaller need only and ran with a workspace 8 bytes short of the query
    ("bf16_ws_workspace_short_of_the_query", (1, 128, 64, 4, 2, 1, 0, 2, 7, 16), "BP_OK with workspace_bytes = query - 8"),
]


def stats_cases():
    """[(tag, case)] of test_gpu_stats_sweep.py: the pinned sweep as it stands, then STATS_EXTRA and STATS_REGRESSIONS."""
    return tagged_cases() + list(STATS_EXTRA) + [("regression:" + t, c) for t, c, _ in STATS_REGRESSIONS]


def counting_inputs(case, index, direction):
    """Operands that make every value a small integer or half-integer, exactly representable in bf16, so that any
    order of additions -- fp32 or double -- is exact.
    direction 0: (x, w): x = 1, no pending activation, w = 1 on the gathered channel index % cin and 0 elsewhere: y is
       the number of taps inside the image, the same in every produced channel.
    direction 1: (dy, w, raw, (scale, shift, slope)): dy = 1, w = 1 on the gathered channel index % cout; raw in {1, 2}
       chequered differently per channel, scale 1, shift -1.5, slope 0.5 (0 on every third channel): t = +-0.5,
       g in {dx, dx / 2, 0} and every term of the three sums is a multiple of 1/4."""
    tr, ci, co, k, s, p, op, n, h, w = case
    wt = np.zeros(weight_shape(case), np.float32)
    if direction == 0:
        g = index % ci
        if tr:
            wt[g, :] = 1.0
        else:
            wt[:, g] = 1.0
        return np.ones((n, ci, h, w), np.float32), wt
    g = index % co
    if tr:
        wt[:, g] = 1.0
    else:
        wt[g, :] = 1.0
    ho, wo = out_shape(case)
    c_, y_, x_ = np.arange(ci)[:, None, None], np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    raw = 1.0 + ((y_ + x_ + c_ + (c_ // 2) * y_ + (c_ // 4) * x_) & 1)
    raw = np.ascontiguousarray(np.broadcast_to(raw[None], (n, ci, h, w)), dtype=np.float32)
    slope = np.full(ci, 0.5, np.float32)
    slope[2::3] = 0.0
    return np.ones((n, co, ho, wo), np.float32), wt, raw, (np.ones(ci, np.float32), np.full(ci, -1.5, np.float32), slope)


def counting_reference(case, direction, T=None):
    """float64 result of the convolution on counting_inputs: the number of taps behind each element (terms() of one
    gathered channel), in every produced channel."""
    tr, ci, co, k, s, p, op, n, h, w = case
    ty, tdx = (terms(case) if T is None else T)[:2]
    if direction == 0:
        return np.ascontiguousarray(np.broadcast_to(ty / ci, (n, co) + ty.shape[2:]))
    return np.ascontiguousarray(np.broadcast_to(tdx / co, (n, ci) + tdx.shape[2:]))


def stats_reference(mode, stored, raw=None, pw=None):
    """float64 per-channel sums the epilogues promise, from a tensor as stored (float64 values of what the device holds,
    NCHW), and the magnitudes behind them.  Returns (sums, mags, g): lists of per-channel arrays.
    mode 1: stored = y: [sum y, sum y^2].
    mode 2 / 3: stored = dx, raw and pw = (scale, shift, slope) float32: t = fma(raw, scale, shift) rounded once to
       float32 decides the mask, g = dx where t > 0, else the float32 product dx * slope (include/bp_hip.h):
       [sum g, sum g raw] and, mode 3, [sum_{t <= 0} dx t]; g is returned for the stored-tensor check of mode 3."""
    ax = (0, 2, 3)
    if mode == 1:
        return [stored.sum(axis=ax), (stored * stored).sum(axis=ax)], [np.abs(stored).sum(axis=ax), (stored * stored).sum(axis=ax)], None
    scale, shift, slope = (np.asarray(v, np.float32)[None, :, None, None] for v in pw)
    r64 = np.asarray(raw, np.float64)
    t = (r64 * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
    prod = (stored.astype(np.float32) * slope).astype(np.float64)        # (fp32 multiply: exact inputs, one rounding)
    g = np.where(t > 0, stored, prod)
    q = [g, g * r64]
    if mode == 3:
        q.append(np.where(t > 0, 0.0, stored * t.astype(np.float64)))
    return [v.sum(axis=ax) for v in q], [np.abs(v).sum(axis=ax) for v in q], g
