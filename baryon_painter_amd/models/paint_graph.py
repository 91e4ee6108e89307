"""The slot format and the capture of the device paint paths (``CVAE.paint_graph``, ``CGAN.paint_graph``).

A captured paint pipeline has two *slots*: input / parameter / output buffer sets, each with its own graph over the same
launch plans.  A slot's per-batch parameters live in ONE uint8 device buffer, its *parameter block*, so that a batch
costs one host-to-device copy; ``ParamBlock`` is the byte layout of that buffer and the typed views over it, on the
device and on a pinned host mirror (``painter._paint_stream_pipeline`` / ``_paint_plane_pipeline``).  A model states the
fields of its block, its buffers and what one replay runs; everything else about a slot and a capture is here.
"""
import torch

from .graph import capture_without_gc


class ParamBlock:
    """Byte layout of ``fields``, an ordered list of (name, torch dtype, shape), each rounded up to 8 bytes:
    ``layout`` name -> (byte offset, dtype, shape) and ``nbytes``.  Needs no GPU."""

    def __init__(self, fields):
        self.layout, self._size, off = {}, {}, 0
        for name, dt, shape in fields:
            shape = tuple(shape)
            self.layout[name] = (off, dt, shape)
            self._size[name] = int(torch.tensor([], dtype=dt).element_size()) * int(torch.Size(shape).numel())
            off += (self._size[name] + 7) // 8 * 8
        self.nbytes = off

    def views(self, buf):
        """name -> typed view of the uint8 tensor ``buf`` (``nbytes`` long): torch views of a device buffer, NumPy views
        of a host buffer.  The views alias ``buf``."""
        if buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() != self.nbytes:
            raise ValueError(f"a parameter block is a flat uint8 tensor of {self.nbytes} bytes")
        out = {}
        for name, (off, dt, shape) in self.layout.items():
            v = buf[off:off + self._size[name]].view(dt).view(shape)
            out[name] = v if buf.is_cuda else v.numpy()
        return out


def paint_fields(n, xf_width, aux_width=1, xf_out_width=None, noise=False, draws=None, parts=1):
    """The fields of a paint pipeline's block for batches of ``n`` tiles: ``xf_in`` / ``xf_out`` (n, xf_width) float64
    parameter rows of the transform and its inverse, ``tile_ids`` (n,) int64, ``seed`` (1,) int64 Philox key, ``aux``
    (n, aux_width) float32 value of the conditioning plane.  Both models carry all five, so that one caller fills either
    model's block.  ``xf_out_width``: the width of ``xf_out`` where it differs (a CVAE with several label fields: the
    fields' rows side by side).  ``noise`` (a pipeline that paints draws from the likelihood, ``bp_likelihood_draw``):
    ``noise_ids`` (n,) int64 and ``noise_org`` (n, 2) int32 {row, col} follow behind the five.  ``draws`` = K (an
    ensemble pipeline, ``CVAE.paint_graph(draws=K)``, whose graph paints its n tiles as ``parts`` sub-batches): the five
    fields are per TILE as ever; with ``noise``, ``noise_ids`` is (parts, K, n / parts) int64 -- per sub-batch the K n /
    parts ids of its samples in the order ``bp_likelihood_draw`` reads them, draw-major -- and there is no ``noise_org``
    (the draws of an ensemble sit at the origin of their lattices).  Without ``draws`` nothing changes."""
    fields = [("xf_in", torch.float64, (n, xf_width)),
              ("xf_out", torch.float64, (n, xf_width if xf_out_width is None else xf_out_width)),
              ("tile_ids", torch.int64, (n,)), ("seed", torch.int64, (1,)), ("aux", torch.float32, (n, aux_width))]
    if noise and draws is not None:
        fields += [("noise_ids", torch.int64, (parts, draws, n // parts))]
    elif noise:
        fields += [("noise_ids", torch.int64, (n,)), ("noise_org", torch.int32, (n, 2))]
    return fields


DRAWS_MAX = 64          # bp_paint_store_moments' limit
DRAW_SHIFT = 40         # draw l of an ensemble draws its pixel noise from the lattice id + (l << DRAW_SHIFT)


def check_draws(draws):
    """``draws`` of an ensemble as an int in 1 ... DRAWS_MAX (ValueError).  Needs no GPU."""
    k = int(draws)
    if k != draws or not 1 <= k <= DRAWS_MAX:
        raise ValueError(f"an ensemble has 1 ... {DRAWS_MAX} draws per tile, got {draws}")
    return k


def ensemble_noise_ids(ids, draws):
    """(draws, n) int64 lattice ids of an ensemble's pixel noise: row l = ``ids`` + (l << 40), so that draw l of a tile
    is what a single painting with that lattice id draws.  ``ids`` (n,) must lie in [0, 2^40) (ValueError).  Needs no
    GPU."""
    import numpy as np
    ids = np.asarray(ids)
    if ids.ndim != 1 or ids.dtype.kind not in "iu":
        raise ValueError(f"noise ids must be a vector of integers, got shape {ids.shape} of {ids.dtype}")
    if len(ids) and (int(ids.min()) < 0 or int(ids.max()) >= 1 << DRAW_SHIFT):
        raise ValueError(f"the noise ids of an ensemble must lie in [0, 2^{DRAW_SHIFT}): bits {DRAW_SHIFT} and above "
                         "number the draws")
    return ids.astype(np.int64)[None, :] + (np.arange(draws, dtype=np.int64) << DRAW_SHIFT)[:, None]


def seed_word(seed):
    """The Philox key ``seed`` (any Python int, taken modulo 2^64) as the int64 a block's ``seed`` field holds."""
    import numpy as np
    return np.array(int(seed) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64).astype(np.int64)


def noise_lattice(ids, origins, n, h, w):
    """``ids`` (n,) int64 and ``origins`` (n, 2) int32 {row, col} (None: None, all zero) of ``bp_likelihood_draw`` for
    ``n`` tiles of ``h`` x ``w`` pixels, as NumPy arrays, checked for what the kernel leaves to its caller: origins are
    not negative, lattice columns stay below 2^24 and rows below 2^31 (ValueError).  Needs no GPU."""
    import numpy as np
    ids = np.asarray(ids)
    if ids.shape != (n,) or ids.dtype.kind not in "iu":
        raise ValueError(f"noise ids must be {n} integers, got shape {ids.shape} of {ids.dtype}")
    ids = ids.astype(np.int64)
    if origins is None:
        org = None
    else:
        org = np.asarray(origins)
        if org.shape != (n, 2) or org.dtype.kind not in "iu":
            raise ValueError(f"noise origins must be ({n}, 2) integers {{row, col}}, got shape {org.shape} of {org.dtype}")
        org = org.astype(np.int64)
        if (org < 0).any():
            raise ValueError("noise origins must not be negative")
        if (org[:, 0] + h > 2 ** 31).any() or (org[:, 1] + w > 2 ** 24).any():
            raise ValueError("the noise lattice has 2^31 rows and 2^24 columns: an origin puts a tile beyond them")
        org = np.ascontiguousarray(org, dtype=np.int32)
    if h > 2 ** 31 or w > 2 ** 24:
        raise ValueError("the noise lattice has 2^31 rows and 2^24 columns: the tile is larger")
    return np.ascontiguousarray(ids), org


def paint_levels(cy, cx, has_p_y_in, L, scales, fields, ensemble, mismatch=ValueError):
    """Which CVAEs the captured paint pipeline takes, in ONE place (``CVAE.paint_graph`` and
    ``CVAEPainter._device_paint_parameters`` both ask here).  ``cy`` = dim_y[0] and ``cx`` = dim_x[0] of the model,
    ``scales`` its split-scale description or None, ``fields`` the number of label fields, ``ensemble`` whether the
    number of draws is the caller's (``paint_graph(draws=K)``) and not the model's ``L``.  Returns the channels of one
    field, ``levels`` = n_scale + include_original (1 without ``scales``), or raises: ``mismatch`` where the model's
    channels are not cy = levels and cx = fields * levels, NotImplementedError for what the pipeline has no step for.
    Needs no GPU."""
    levels = 1 if scales is None else int(scales["n_scale"]) + int(bool(scales["include_original"]))
    if cy != levels or cx != fields * levels:
        raise mismatch(f"the captured paint pipeline paints {fields} label field(s) of {levels} channel(s) from tiles of "
                       f"{levels} channel(s) (a split-scale transform's levels, or 1): it needs dim_y[0] = {levels} and "
                       f"dim_x[0] = {fields * levels}, the model has {cy} and {cx}")
    if scales is not None and has_p_y_in:
        raise NotImplementedError("the captured paint pipeline has no split-scale load step for a p_y_in network "
                                  "(bp_paint_load_scales2 writes two destinations); paint / paint_batch take it")
    if L != 1 and not ensemble:
        raise NotImplementedError("the captured paint pipeline needs L = 1 (sample_P, paint and paint_batch take any L: "
                                  "they paint with one latent draw per tile)")
    return levels


def new_slot(raw_shape, out_shape, block, device):
    """One slot: ``raw``, ``out``, the uint8 ``block`` and its named views, ``xf_in`` / ``xf_out`` filled with 1.0 (a
    valid transform for the warm-up).  ``out_shape`` may be a dict name -> shape of several outputs in place of ``out``
    (an ensemble's ``mean`` / ``var`` / ``draws``)."""
    outs = out_shape if isinstance(out_shape, dict) else {"out": out_shape}
    sl = {"raw": torch.zeros(raw_shape, device=device), "block": torch.zeros(block.nbytes, device=device, dtype=torch.uint8)}
    sl.update({name: torch.zeros(shape, device=device) for name, shape in outs.items()})
    sl.update(block.views(sl["block"]))
    sl["xf_in"].fill_(1.0)
    sl["xf_out"].fill_(1.0)
    return sl


def fork_join(part, parts, device):
    """``run(sl)`` for ``capture``: ``part(k, sl)`` for k < ``parts``, part 0 on the current stream and part k > 0 on a
    side stream of its own -- the side streams wait on the main stream, run their parts, and the main stream waits on all
    of them, so that inside one graph the parts are parallel branches."""
    others = [torch.cuda.Stream(device=device) for _ in range(parts - 1)]

    def run(sl=None):
        main = torch.cuda.current_stream(device)
        for k, s2 in enumerate(others, 1):
            s2.wait_stream(main)
            with torch.cuda.stream(s2):
                part(k, sl)
        part(0, sl)
        for s2 in others:
            main.wait_stream(s2)
    return run


def capture(run, slots, device):
    """``run(slots[0])`` once outside capture on a side stream (packs weights, sizes workspaces), then one graph per
    slot, captured on that stream in the order of ``slots``; a slot that is a dict gets its graph as ``"graph"``.
    Returns the graphs.  ``slots`` is ``[None]`` where what is captured has no slots."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side), torch.no_grad():
        run(slots[0])
    torch.cuda.current_stream(device).wait_stream(side)
    graphs = []
    for sl in slots:
        graph = torch.cuda.CUDAGraph()
        # (thread-local capture: under data parallelism the process group's watchdog thread may query events
        #  while this thread captures; that is harmless and must not invalidate the capture)
        with torch.no_grad(), capture_without_gc(), \
                torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            run(sl)
        graphs.append(graph)
        if sl is not None:
            sl["graph"] = graph
    return graphs
