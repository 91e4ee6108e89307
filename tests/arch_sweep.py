"""The architectures of the layer-language sweep (plain module, no test in here; imports without a GPU and without the
reference).  tests/test_arch_sweep_host.py checks the list itself on the CPU, tests/test_gpu_arch_sweep.py runs every
entry through the plan compiler (``models/graph.py``, ``models/cvae.py``) against the float64 evaluation of the same
layer lists (``oracle/torch_ref.py``).

``cases()`` -> [(tag, architecture, n, alpha_var)]: 24 Type-1 CVAEs on 64^2 tiles (three on 32^2), batch 2 or 3, every
ReLU softened to LeakyReLU(0.9) and every PReLU slope at 0.9 (``syn.softened_architecture`` / ``syn.soften_params``).
Everything is a fixed table and no generator is drawn from: a block whose table entry leaves its (bias, batch-norm,
activation) triple open takes the triple that has stood least often so far in front of the kind of layer behind it
(``_Builder``), which is how the list comes to hold every triple in front of every kind.

The table is written in a small shorthand, one token per block:
    C(cout, s, k, f)   convolution block           s: scale 1 / 2 / 4, k: odd kernel at scale 1
    T(cout, s, k, f)   transposed-convolution block
    R(kind)            residual block on the current width: "relu" (``arch.res_block``), "leaky"
                       (``arch.leaky_res_block``), "notail" (no activation behind the sum), "nobn" (branch without
                       batch-norm), "prelu" (PReLU inside the branch), "bias" (biased convolutions inside the branch)
    f: three characters  bias "b" / "-",  batch-norm "n" / "-",  activation "0" none / "r" ReLU / "l" leaky / "p" PReLU;
       None: filled in (see above).
``BF16`` names the entries that run with ``CVAE(dtype="bf16")`` (``BF16_NOT_RUN``: the two built for it that do not, and
why); ``REFUSED`` / ``REFUSED_BF16`` are the candidates the language refuses when the plan is built, with the layer the
NotImplementedError has to name; ``REFUSED_BF16_AT_BACKWARD`` those the bf16 kernels refuse at the first backward pass.
``SEEDS``: the data seed of a case where it is not the common one, and why."""
import numpy as np

from baryon_painter_amd.models import arch as A
from baryon_painter_amd.utils import synthetic as syn

SLOPE = 0.9
LEAKY = 0.8                                  # slope of the blocks written as "leaky relu" (distinct from the softened ReLUs)
SEED_W, SEED_D, SEED_EPS = 7, 1234, 99
TRIPLES = [b + n + a for b in "b-" for n in "n-" for a in "0rlp"]
NEXT_KINDS = ("conv", "transp conv", "residual block", "end")
NETS = (("q_x_in", "q_x_in"), ("q_y_in", "q_y_in"), ("q_x_y_out", "q_out"), ("p_y_in", "p_y_in"), ("p_z_in", "p_z_in"),
        ("p_y_z_in", "p_y_z_in"), ("prior_z_y", "prior_network"))


def C(cout, s=1, k=3, f=None):
    return ("conv", cout, s, k, f)


def T(cout, s=2, k=3, f=None):
    return ("transp conv", cout, s, k, f)


def R(kind="relu"):
    return ("res", kind)


_ACT = {"0": None, "r": "relu", "l": "leaky relu", "p": "prelu"}


def _res(kind, c):
    body, tail = A.leaky_res_block(c, LEAKY) if kind == "leaky" else A.res_block(c)
    body = list(body)
    if kind == "notail":
        tail = (None,)
    elif kind == "nobn":
        body = [body[0], body[2], body[3]]
    elif kind == "prelu":
        body[2] = ("prelu",)
    elif kind == "bias":
        for i in (0, 3):
            body[i] = (body[i][0], dict(body[i][1], bias=True))
    elif kind not in ("relu", "leaky"):
        raise ValueError(kind)
    return ("residual block", (body, tail))


class _Builder:
    """Turns token lists into layer lists.  A block whose table entry leaves its triple open takes the triple that has
    so far stood least often in front of the kind of layer that follows it (ties: the order of TRIPLES) -- counted over
    everything built before it, so the table below fills the pair table by construction and stays a fixed list."""

    def __init__(self, counts=None):
        self.counts = {} if counts is None else counts

    def triple(self, f, nxt, nobias, quiet):
        if f is None:
            open_ = [t for t in TRIPLES if not (nobias and t[0] == "b") and not (t[:2] == "bn" and not quiet)]
            f = min(open_, key=lambda t: (self.counts.get((t, nxt), 0), TRIPLES.index(t)))
        self.counts[(f, nxt)] = self.counts.get((f, nxt), 0) + 1
        return f

    def chain(self, cin, spec, nobias=False, quiet=0):
        """``quiet``: the number of leading blocks that may be filled with a bias in front of a batch-norm.  The true
        gradient of such a bias is zero and what an fp32 execution leaves there is the rounding of a sum over the
        pixels; only where little gradient flows (the prior network) in a net whose largest
        gradient is large (the rows marked ``bn_bias``) does the stock fp32 evaluation stay inside what the host test
        allows it.  Written out in the table, such a block stands anywhere."""
        layers, c = [], cin
        for i, tok in enumerate(spec):
            if tok[0] == "res":
                layers.append(_res(tok[1], c))
                continue
            kind, cout, s, k, f = tok
            nxt = "end" if i + 1 == len(spec) else "residual block" if spec[i + 1][0] == "res" else spec[i + 1][0]
            f = self.triple(f, nxt, nobias, i < quiet)
            layers += A.conv_block(c, cout, type=kind, scale=s, kernel=k, bias=f[0] == "b", batchnorm=f[1] == "n",
                                   activation=_ACT[f[2]], relu_slope=LEAKY)
            c = cout
        return layers, c


def _build(b, size, trunk, heads, qx, qy, qo, prior, pz, py=None, zs=None, L=1, n_fields=1, n_scale=1,
           bf16=False, bn_bias=False):
    """One architecture from its table row.  ``qo`` / ``prior`` end in the 2 * dim_z[0] latent channels, ``heads`` in
    the n_fields * n_scale output channels; the channel counts in between come from the tokens."""
    zs = size // 32 if zs is None else zs
    n_x, cy = n_fields * n_scale, n_scale + 1
    a = {"type": "Type-1", "dim_x": (n_x, size, size), "dim_y": (n_scale, size, size), "dim_z": (1, zs, zs),
         "n_x_features": n_x, "aux_label": True, "min_x_var": 1e-7, "min_z_var": 1e-7, "L": L}
    a["q_x_in"], cqx = b.chain(n_x, qx)
    a["q_y_in"], cqy = b.chain(cy, qy)
    a["q_x_y_out"] = b.chain(cqx + cqy, qo)[0] + [("unflatten", (2, 1, zs, zs))]
    if prior is not None:
        a["prior_z_y"] = b.chain(cy, prior, quiet=9 * bn_bias)[0] + [("unflatten", (2, 1, zs, zs))]
    c_hy = cy
    a["p_y_in"] = None
    if py is not None:
        a["p_y_in"], c_hy = b.chain(cy, py)
    a["p_z_in"], c_hz = b.chain(1, pz)
    a["p_y_z_in"], c = b.chain(c_hz + c_hy, trunk, nobias=bf16)
    out = []
    for h in heads:
        first, _ = b.chain(c, h[:1], nobias=bf16)
        out.append(first + b.chain(h[0][1], h[1:])[0])
    a["p_y_z_out"] = tuple(out)
    return a


def _softplus(head):
    return list(head) + [("softplus",)]


# ------------------------------------------------------------------------------------------------------- the table
# stride orders of the recognition / prior nets (product 32 at dim_z = size / 32)
def _down(widths, scales, fs=None):
    fs = fs or [None] * len(widths)
    return [C(c, s, 3, f) for c, s, f in zip(widths, scales, fs)]


def _up(widths, scales, fs=None):
    fs = fs or [None] * len(widths)
    return [T(c, s, 3, f) for c, s, f in zip(widths, scales, fs)]


def _prior_res(first, second, k):
    """A prior network with a residual block behind each of its first two levels, and one level up and down again
    at its end (the slots in which a block stands in front of a residual block / a transposed convolution)."""
    return [C(8, 2), R(first), C(16, 4), R(second), C(32, 4), T(16, 2), C(16, 2), C(2, 1, k)]


_HEAD3 = [C(8, 1, 7, "--p"), C(1, 1, 5, "--p"), C(1, 1, 3, "--0")]          # the fiducial head
_Q = dict(qx=_down([8, 16, 32], [2, 4, 4]), qy=_down([8, 16, 32], [2, 4, 4]), qo=[C(2, 1, 5)],
          prior=_down([8, 16, 32], [2, 4, 4]) + [C(2, 1, 5)], pz=_up([1, 1, 1], [2, 4, 4], ["-nr"] * 3))

_TABLE = [
    # tag, size, n, alpha_var, keyword arguments of _build
    ("stem12_bias_leaky", 64, 2, 1.0, dict(
        trunk=[C(12, 1, 5, "b-l"), C(24, 2), C(48, 2), C(48, 1, 1, "--p"), C(48, 1, 3, "-n0"), R("relu"), T(24, 2),
               T(12, 2, 3, "-nr")],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "b-p"), C(1, 1, 3, "b-0")]], **_Q)),
    ("k7_stem_scale4", 64, 2, 0.3, dict(
        trunk=[C(16, 1, 7, "--r"), C(32, 4, 3, "-nl"), C(32, 1, 1, "--p"), R("leaky"), T(16, 4, 3, "-nr")],
        heads=[_HEAD3, [C(8, 1, 7, "--p"), C(1, 1, 5, "--p"), C(1, 1, 3, "--0")]],
        qx=[C(8, 2, 3, "--l"), C(16, 4), C(32, 4)], qy=_down([6, 12, 24], [4, 4, 2]), qo=[C(2, 1, 5)],
        prior=_down([4, 8, 16, 32], [2, 2, 2, 4]) + [C(2, 1, 3)], pz=_up([1, 1, 1], [4, 4, 2], ["-nr", "-n0", "-nl"]))),
    ("res_first", 64, 2, 1.0, dict(
        trunk=[R("relu"), C(16, 1, 5, "-nr"), C(32, 2), R("notail"), T(16, 2, 3, "-nl")],
        heads=[[C(8, 1, 7, "-np"), C(1, 1, 3, "--0")]],
        qx=_down([4, 8, 16], [4, 2, 4]), qy=[C(8, 4), C(16, 2), R("relu"), C(32, 4)], qo=[C(2, 1, 3)],
        prior=[C(8, 4), C(16, 2), R("leaky"), C(32, 4), C(2, 1, 1)], pz=_up([2, 2, 1], [2, 4, 4]))),
    ("res_last_two_heads", 64, 3, 1.0, dict(
        trunk=[C(16, 1, 3), C(64, 2, 3, "--l"), R("relu"), T(16, 2, 3, "b-r"), R("nobn")],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--0")], [C(4, 1, 5, "b-l"), C(1, 1, 3, "--0")]],
        bn_bias=True, **dict(_Q, pz=_up([3, 2, 1], [2, 4, 4], ["b-r", "--p", "b-0"]), prior=_prior_res("relu", "leaky", 5)))),
    ("depth3_k9", 64, 2, 1.0, dict(
        trunk=[C(8, 1, 9), C(16, 2), C(32, 2), C(64, 2), T(32, 2), T(16, 2), T(8, 2), C(6, 1, 9)],
        heads=[[C(1, 1, 5, "--0")]], **dict(_Q, prior=None, qy=[C(8, 2), C(16, 4), R("notail"), C(32, 4)],
                                            qx=[C(8, 2), C(16, 4), C(16, 1, 3), R("relu"), C(32, 4)]))),
    ("fields2", 64, 2, 0.3, dict(
        trunk=[C(16, 1, 5), C(32, 2), R("relu"), R("prelu"), T(16, 2)],
        heads=[[C(8, 1, 7), C(2, 1, 5), C(2, 1, 3, "b-0")], [C(8, 1, 7), C(2, 1, 3, "--0")]], n_fields=2, bn_bias=True,
        **dict(_Q, prior=_prior_res("bias", "relu", 3)))),
    ("scales2", 64, 2, 1.0, dict(
        trunk=[C(12, 1, 3), C(24, 2), C(24, 1, 7), T(6, 2)],
        heads=[[C(4, 1, 5), C(2, 1, 5, "-n0"), C(2, 1, 3, "--0")]], n_scale=2,
        **dict(_Q, pz=_up([1, 2, 1], [2, 4, 4])))),
    ("fields2_scales2", 64, 2, 1.0, dict(
        trunk=[C(16, 1, 3), C(16, 4), T(16, 4), C(8, 1, 5)],
        heads=[[C(8, 1, 3), C(4, 1, 1, "b-0")], [C(4, 1, 3), C(4, 1, 5, "--0")]], n_fields=2, n_scale=2, bn_bias=True,
        **dict(_Q, qy=_down([8, 16, 32, 32], [2, 2, 2, 4]), prior=_prior_res("notail", "relu", 1)))),
    ("L2_pyin", 64, 2, 1.0, dict(
        trunk=[C(16, 1, 5), C(32, 2), R("leaky"), T(16, 2)], heads=[_HEAD3], L=2, py=[C(4, 1, 3, "-nr")], **_Q)),
    ("L2_two_heads", 64, 2, 0.3, dict(
        trunk=[C(8, 1, 3), C(24, 2), C(24, 1, 5), T(8, 2)],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--0")], [C(2, 1, 3), C(1, 1, 3, "--0")]], L=2, **_Q)),
    ("pyin_no_act", 64, 3, 1.0, dict(
        trunk=[C(16, 1, 3), C(48, 4), R("relu"), T(12, 4), C(16, 1, 1)],
        heads=[[C(8, 1, 7, "-nr"), C(1, 1, 5, "--p"), C(1, 1, 3, "--0")]],
        py=[C(6, 1, 5, "b-l"), C(3, 1, 3, "-n0")], **_Q)),
    ("pyin_two_heads", 64, 2, 1.0, dict(
        trunk=[C(32, 1, 3), C(64, 2), T(32, 2), C(16, 1, 7)],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--0")], [C(8, 1, 7, "--r"), C(1, 1, 5, "--0")]],
        py=[C(2, 1, 1, "--p")], **dict(_Q, pz=_up([4, 2, 2], [4, 2, 4], ["-nr", "--l", "-n0"])))),
    ("dimz4_two_levels", 64, 2, 1.0, dict(
        trunk=[C(16, 1, 3), C(32, 2), C(64, 2), R("relu"), R("leaky"), T(32, 2), T(16, 2)],
        heads=[_HEAD3], zs=4, qx=_down([8, 32], [4, 4]), qy=_down([4, 8, 32], [2, 2, 4]), qo=[C(2, 1, 5)],
        prior=_down([8, 16], [4, 4]) + [C(2, 1, 3)], pz=_up([2, 1], [4, 4], ["b-l", "-nr"]))),
    ("narrow", 64, 3, 1.0, dict(
        trunk=[C(1, 1, 3), C(2, 2), C(3, 2), C(4, 1, 5), R("relu"), T(6, 2), T(2, 2)],
        heads=[[C(3, 1, 3), C(1, 1, 1, "--0")]],
        qx=_down([1, 2, 3], [2, 4, 4]), qy=_down([3, 4, 6], [4, 4, 2]), qo=[C(2, 1, 1)],
        prior=[C(2, 4), C(3, 2), R("relu"), C(4, 4), C(2, 1, 5)], pz=_up([1, 1, 1], [4, 2, 4]))),
    ("wide128", 64, 2, 1.0, dict(
        trunk=[C(32, 1, 3), C(128, 4), R("relu"), C(128, 1, 1), T(32, 4), T(12, 1, 5)],
        heads=[[C(8, 1, 7), C(1, 1, 5, "--0")]], **dict(_Q, pz=_up([2, 2, 1], [2, 4, 4], ["--l", "-nr", "-nr"])))),
    # ---- 32^2 tiles (dim_z 1 x 1): most layers below one kernel tile; no batch-norm at the 1 x 1 levels
    ("s32_plain", 32, 3, 1.0, dict(
        trunk=[C(16, 1, 5), C(32, 2), R("relu"), T(16, 2)], heads=[_HEAD3],
        qx=_down([8, 16, 32], [2, 4, 4], [None, None, "--l"]), qy=_down([8, 16, 32], [4, 2, 4], [None, None, "b-r"]),
        qo=[C(2, 1, 1, "b-0")], prior=_down([8, 16, 32], [4, 4, 2], [None, None, "--p"]) + [C(2, 1, 1, "--0")],
        pz=_up([2, 1, 1], [2, 4, 4], ["--l", None, None]))),
    ("s32_two_heads", 32, 2, 0.3, dict(
        trunk=[C(12, 1, 3), C(24, 4), T(12, 4), C(8, 1, 7)],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--0")], [C(4, 1, 3), C(1, 1, 3, "b-0")]],
        qx=_down([4, 8, 16], [4, 4, 2], [None, None, "--r"]), qy=_down([4, 8, 16], [2, 4, 4], [None, None, "--0"]),
        qo=[C(2, 1, 1, "--0")], prior=None, pz=_up([1, 1, 1], [4, 4, 2], ["b-r", None, None]))),
    ("s32_bf16", 32, 3, 1.0, dict(
        trunk=[C(8, 1, 3), C(16, 2), C(32, 2), T(16, 2), T(8, 2)],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--p"), C(1, 1, 3, "b-0")]], bf16=True,
        qx=_down([8, 16, 32], [2, 4, 4], [None, None, "--l"]), qy=_down([8, 16, 32], [2, 4, 4], [None, None, "--l"]),
        qo=[C(2, 1, 1, "--0")], prior=_down([8, 16, 32], [2, 4, 4], [None, None, "--r"]) + [C(2, 1, 1, "b-0")],
        pz=_up([1, 1, 1], [2, 4, 4], ["--r", None, None]))),
    # ---- the bf16 stratum (64^2): no bias in the trunk and in the heads' first two layers, bf16-capable geometries
    ("bf16_fid_like", 64, 2, 0.3, dict(
        trunk=[C(16, 1, 5, "-nr"), C(32, 2), C(64, 2, 3, "--p"), C(128, 2, 3, "-n0"), R("relu"), R("leaky"), T(64, 2),
               T(32, 2, 3, "--l"), T(16, 2)],
        heads=[_HEAD3, _HEAD3], bf16=True, **dict(_Q, pz=_up([4, 2, 1], [2, 4, 4], ["-nr", "-nr", "--l"])))),
    ("bf16_fp32_stem", 64, 2, 1.0, dict(
        trunk=[C(24, 1, 5), C(48, 2), C(64, 1, 3), C(128, 2), R("relu"), T(64, 2), T(16, 2), C(16, 1, 7)],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--0")]], bf16=True,
        **dict(_Q, pz=_up([2, 2, 1], [4, 2, 4], ["--p", "-nr", "-n0"])))),
    ("bf16_scale4", 64, 3, 1.0, dict(
        trunk=[C(8, 1, 3), C(32, 4), R("notail"), T(8, 4), C(16, 1, 7)],
        heads=[_HEAD3, [C(8, 1, 7, "--l"), C(1, 1, 5, "--0")]], bf16=True,
        **dict(_Q, pz=_up([2, 2, 1], [2, 4, 4], ["--l", "-nr", "-nr"])))),
    ("bf16_no_res", 64, 2, 1.0, dict(
        trunk=[C(16, 1, 7, "--l"), C(16, 1, 5), C(32, 2), T(16, 2), C(8, 1, 3)],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--p"), C(1, 1, 3, "b-0")]], bf16=True, **_Q)),
    ("bf16_wide", 64, 3, 0.3, dict(
        trunk=[C(64, 1, 3), C(128, 2), R("relu"), R("leaky"), T(64, 2), C(16, 1, 3)],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--0")], [C(8, 1, 7, "--r"), C(1, 1, 5, "--0")]], bf16=True, bn_bias=True,
        **dict(_Q, prior=_prior_res("relu", "prelu", 5), pz=_up([2, 2, 1], [2, 4, 4], ["--l", "-nr", "-nr"])))),
    ("bf16_transp_s1", 64, 2, 1.0, dict(
        trunk=[C(16, 1, 5), C(64, 2), R("relu"), T(16, 2), T(16, 1, 3)],
        heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--p"), C(1, 1, 3, "--0")]], bf16=True,
        **dict(_Q, pz=_up([3, 2, 1], [4, 4, 2], ["b-r", "-nl", "--0"])))),
]
# Rows built for the bf16 policy that are not run with dtype="bf16", and why; and one more that the policy compiles
# although its stem is biased (the stem then stays an fp32 layer between fp32 slots).
BF16_NOT_RUN = {
    "bf16_scale4": "the transposed scale-4 layer (32 -> 8) has no bf16 weight gradient (REFUSED_BF16_AT_BACKWARD)",
    "bf16_wide": "its prior network holds biases in front of batch-norms: their true gradient is exactly zero and the "
                 "rounding twin's relative distance is undefined for them",
}
BF16 = tuple(row[0] for row in _TABLE if row[4].get("bf16") and row[0] not in BF16_NOT_RUN) + ("s32_plain",)


def raw_architectures():
    """[(tag, architecture as the table writes it -- ReLUs not yet softened --, n, alpha_var)]."""
    out = []
    b = _Builder()
    for tag, size, n, alpha, kw in _TABLE:
        a = _build(b, size, **kw)
        a["p_y_z_out"] = (_softplus(a["p_y_z_out"][0]),) + tuple(a["p_y_z_out"][1:])
        out.append((tag, a, n, alpha))
    return out


_CASES = []


def cases():
    if not _CASES:
        _CASES.extend((tag, syn.softened_architecture(a, SLOPE), n, alpha) for tag, a, n, alpha in raw_architectures())
    return list(_CASES)


def case(tag):
    return next(c for c in cases() if c[0] == tag)


# ------------------------------------------------------------------------------------------------------- refusals
def _refused():
    """[(tag, architecture, n, dtype, pattern the NotImplementedError must match)]: candidates the plan compiler refuses
    when it builds the training plan of the architecture."""
    out = []
    base = dict(_TABLE[0][4])
    # a branch that is concatenated must end in a convolution: a residual block cannot write a channel slice
    kw = dict(base, qx=_down([8, 16, 32], [2, 4, 4]) + [R("relu")])
    out.append(("res_ends_q_x_in", _build(_Builder(), 64, **kw), 2, "f32", r"residual block as the last layer of a concat"))
    kw = dict(base, pz=_up([1, 1, 1], [2, 4, 4], ["-nr"] * 3) + [R("relu")])
    out.append(("res_ends_p_z_in", _build(_Builder(), 64, **kw), 2, "f32", r"residual block as the last layer of a concat"))
    # a head ends in a bare convolution
    kw = dict(base, heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "-n0")]])
    out.append(("bn_ends_head", _build(_Builder(), 64, **kw), 2, "f32", r"a head must end in conv"))
    kw = dict(base, heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "--p")]])
    out.append(("prelu_ends_head", _build(_Builder(), 64, **kw), 2, "f32", r"a head must end in conv"))
    # bf16: a layer the bf16 kernels do not take (width 24 / 48, a bias, a batch-norm that moves the head's second
    # convolution off the policy's index) behind a bf16 slot
    bf = dict(_TABLE[[r[0] for r in _TABLE].index("bf16_no_res")][4])
    kw = dict(bf, trunk=[C(16, 1, 3, "-nr"), C(24, 1, 3, "-nr"), C(16, 1, 3, "-nr")])
    out.append(("bf16_width24", _build(_Builder(), 64, **kw), 2, "bf16", r"p_y_z_in\.3: an fp32 layer cannot read a bf16"))
    kw = dict(bf, trunk=[C(16, 1, 3, "-nr"), C(32, 2, 3, "-nr"), T(48, 2, 3, "-nr"), C(16, 1, 3, "-nr")])
    out.append(("bf16_width48", _build(_Builder(), 64, **kw), 2, "bf16", r"p_y_z_in\.6: an fp32 layer cannot read a bf16"))
    kw = dict(bf, heads=[[C(8, 1, 7, "--p"), C(1, 1, 5, "b-p"), C(1, 1, 3, "--0")]])
    out.append(("bf16_bias_head", _build(_Builder(), 64, **kw), 2, "bf16", r"p_mu_out\.2: an fp32 layer cannot read a bf16"))
    kw = dict(bf, heads=[[C(8, 1, 7, "-np"), C(1, 1, 5, "--p"), C(1, 1, 3, "--0")]])
    out.append(("bf16_bn_head", _build(_Builder(), 64, **kw), 2, "bf16", r"p_mu_out\.3: an fp32 layer cannot read a bf16"))
    kw = dict(bf, trunk=[C(24, 1, 3, "-nr"), C(32, 1, 3, "-nr"), R("relu"), C(16, 1, 3, "-nr")])
    out.append(("bf16_res_after_fp32", _build(_Builder(), 64, **kw), 2, "bf16", r"p_y_z_in\.6: an fp32 layer cannot read|"
                r"p_y_z_in\.\d+: residual branch and skip differ"))
    # bf16: geometries the bf16 policy takes by shape when the plan is built, but for which the bf16 kernels have no
    # backward on the views they get -- refused only at the first backward pass (RuntimeError naming the layer):
    # a k1 layer, the 8 -> 16 k9 layer and the transposed scale-4 layer 32 -> 8 (no bf16 weight gradient); a head whose
    # second convolution is not 8 -> 1 k5 (the one data gradient with a kernel of its own) -- 8 -> 1 k3, 4 -> 1 k5,
    # 8 -> 2 k5 (n_fields = 2)
    kw = dict(bf, trunk=[C(16, 1, 7, "--l"), C(16, 1, 1, "-nr"), C(8, 1, 3, "-nr")])
    out.append(("bf16_k1", _build(_Builder(), 64, **kw), 2, "bf16@backward", r"p_y_z_in\.2 backward_weight failed: shape not"))
    kw = dict(bf, trunk=[C(8, 1, 3, "-nr"), C(32, 4, 3, "-nr"), T(8, 4, 3, "-nr"), C(8, 1, 3, "-nr")])
    out.append(("bf16_transp_scale4", _build(_Builder(), 64, **kw), 2, "bf16@backward",
                r"p_y_z_in\.6 backward_weight failed: shape not"))
    kw = dict(bf, trunk=[C(8, 1, 3, "-nr"), C(16, 1, 9, "-nr")])
    out.append(("bf16_k9", _build(_Builder(), 64, **kw), 2, "bf16@backward", r"p_y_z_in\.3 backward_weight failed: shape not"))
    for tag, head, nf in (("bf16_head_k3", [C(8, 1, 5, "--l"), C(1, 1, 3, "--0")], 1),
                          ("bf16_head_4", [C(4, 1, 3, "--r"), C(1, 1, 5, "--0")], 1),
                          ("bf16_head_fields2", [C(8, 1, 7, "--p"), C(2, 1, 5, "--0")], 2)):
        kw = dict(bf, trunk=[C(16, 1, 3, "-nr")], heads=[head], n_fields=nf)
        out.append((tag, _build(_Builder(), 64, **kw), 2, "bf16@backward", r"p_mu_out\.2 backward_data failed: shape not"))
    fixed = []
    for tag, a, n, dt, pat in out:
        a["p_y_z_out"] = (_softplus(a["p_y_z_out"][0]),) + tuple(a["p_y_z_out"][1:])
        fixed.append((tag, syn.softened_architecture(a, SLOPE), n, dt, pat))
    return fixed


REFUSED = [r for r in _refused() if r[3] == "f32"]
REFUSED_BF16 = [r for r in _refused() if r[3] == "bf16"]
REFUSED_BF16_AT_BACKWARD = [r for r in _refused() if r[3] == "bf16@backward"]


# ------------------------------------------------------------------------------------------------------- helpers
def net_lists(arch):
    """(architecture key, state-dict prefix, layer list) of every net the architecture has."""
    out = [(key, attr + ".", arch.get(key)) for key, attr in NETS]
    out += [(f"p_y_z_out[{i}]", ("p_mu_out.", "p_var_out.")[i], seq) for i, seq in enumerate(arch["p_y_z_out"][:2])]
    return [(k, p, list(seq)) for k, p, seq in out if seq]


def blocks(seq):
    """The conv-like layers of a list as [(kind, triple or None, config)]: kind "conv" / "transp conv" with the block's
    (bias, batch-norm, activation) triple in the shorthand above, or "residual block"."""
    out, i = [], 0
    names = [layer[0].lower() for layer in seq]
    while i < len(seq):
        if names[i] in ("conv", "transp conv"):
            cfg, j = seq[i][1], i + 1
            bn = j < len(seq) and names[j] == "batchnorm"
            j += bn
            act = names[j] if j < len(seq) and names[j] in ("relu", "leaky relu", "prelu") else None
            f = ("b" if cfg["bias"] else "-") + ("n" if bn else "-") + {None: "0", "relu": "r", "leaky relu": "l",
                                                                         "prelu": "p"}[act]
            out.append((names[i], f, cfg))
        elif names[i] == "residual block":
            out.append(("residual block", None, seq[i][1]))
        i += 1
    return out


def pair_table(architectures):
    """{(triple, kind of the next conv-like layer or "end"): count} over every convolution block of every net, from
    the layer lists as written (before softening)."""
    table = {}
    for a in architectures:
        for _, _, seq in net_lists(a):
            bl = blocks(seq)
            for (kind, f, _), nxt in zip(bl, bl[1:] + [("end", None, None)]):
                if f is not None:
                    table[(f, nxt[0])] = table.get((f, nxt[0]), 0) + 1
    return table


def axes(architectures):
    """What the list holds on the other axes: sets of widths, kernels at scale 1, (kind, scale) of the rest."""
    widths, kernels, strided, res = set(), set(), set(), set()
    for a in architectures:
        for _, _, seq in net_lists(a):
            for kind, f, cfg in blocks(seq):
                if f is None:
                    body, tail = cfg
                    res.add((len(body), tail[0]))
                    continue
                widths.add(cfg["out_channels"])
                if cfg["stride"] == 1:
                    kernels.add(cfg["kernel_size"])
                else:
                    strided.add((kind, cfg["stride"]))
    return {"widths": widths, "kernels": kernels, "strided": strided, "residual": res}


def param_shapes(arch):
    from oracle.cvae_oracle import CVAEOracle
    return CVAEOracle(arch, dtype=np.float64).param_shapes()


def parameters(arch):
    """Seeded weights, PReLU slopes at SLOPE."""
    return syn.soften_params(syn.fill_params(param_shapes(arch), SEED_W), SLOPE)


# Data seeds of the cases that do not take SEED_D.  A case is only as good as its distance from the activations' kinks:
# on these small tiles a single mask that an fp32 execution takes the other way than the float64 graph changes
# d(loss)/d(raw) of a whole layer by (1 - slope) / sqrt(elements) -- 4e-4 for the 50 000 elements of a six-channel 64^2
# layer, above the sweep's limit of 3e-4.  Measured on the first list: every run that missed that limit had exactly one
# such mask (an activation input within fp32 rounding of zero), every run that met it none.  With a million activation
# inputs per case no margin can be asked of all of them on the host, so the GPU test counts the masks of each run
# (``mask_flips``) and a case in which a run has one takes the next seed (+20) in which none has.
SEEDS = {"res_last_two_heads": 1254, "depth3_k9": 1254, "fields2_scales2": 1254, "bf16_fid_like": 1254,
         "bf16_fp32_stem": 1254, "bf16_scale4": 1254, "bf16_no_res": 1274}


def data_seed(tag):
    return SEEDS.get(tag, SEED_D)


def inputs(arch, n, seed=SEED_D):
    """(x, y, aux, eps, zfix): x with dim_x[0] and y with dim_y[0] channels (one synthetic batch per channel, seeds
    seed + 10 j; aux of the first), eps for L draws."""
    size, zs = arch["dim_x"][1], arch["dim_z"][1:]
    xs, ys, aux = [], [], None
    for j in range(max(arch["dim_x"][0], arch["dim_y"][0])):
        x, y, a = syn.synthetic_batch(n, size, size, seed=seed + 10 * j)
        xs.append(x)
        ys.append(y)
        aux = a if aux is None else aux
    x = np.concatenate(xs[:arch["dim_x"][0]], axis=1)
    y = np.concatenate(ys[:arch["dim_y"][0]], axis=1)
    eps = syn.synthetic_eps((arch.get("L", 1), n, 1, *zs), seed=seed - SEED_D + SEED_EPS)
    zfix = syn.synthetic_eps((n, 1, *zs), seed=101)
    return x, y, aux, eps, zfix


def scale_floors(truth):
    """name -> 1e-4 x the largest gradient magnitude among the multi-element tensors of the net (the scale floor of
    tests/test_gpu_cgan.py, where the net is the generator or the discriminator; here it is the CVAE); ``truth``:
    name -> float64 gradient."""
    top = max(float(np.abs(v).max()) for v in truth.values() if np.size(v) > 1)
    return {k: 1e-4 * top for k in truth}


def distance(a, b, floor):
    """max |a - b| / max(max |b|, floor)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-300))
