"""Tile datasets that feed ``CVAEPainter.train`` / ``validate``.

``BAHAMASDataset`` keeps the reference's public surface and its sample-index -> tile mapping
(/root/reference/baryon_painter/utils/datasets.py:15-508) -- including the mapping's quirks,
which define "bit-exact tile indexing":
  * the (stack, tile) part of the index is taken ``% n_tile_permutation**2`` (datasets.py:327),
    so with permutations on only 64 (stack, tile) combinations are ever visited and with
    permutations off only the first;
  * flip code 3 is a no-op (duplicated ``elif flip_idx == 2``, datasets.py:353-358);
  * ``get_batch`` multiplies the drawn indices by ``len(redshifts)`` (datasets.py:459).
``fixed_indexing=True`` opts out of the first two.

``SyntheticTileDataset`` implements the same protocol on seeded synthetic tiles (no files).
"""
import collections
import copy
import ctypes as C
import os

import numpy as np

from . import synthetic as syn

# dark-matter mass -> SLICS delta-plane units (datasets.py:301-302, 399)
def slics_scale(n_grid):
    return 1 / (n_grid / 8 * 5) * 0.2793 / (0.2793 - 0.0463)


def _identity(x, field, z, stats):
    return x


class _Compiled:
    """``f(x, field=..., z=...)`` with the transform and statistics bound (datasets.py:8-13);
    a class instead of a lambda so that checkpoints pickle without dill's closure support."""

    def __init__(self, transform, stats, field=None, z=None):
        self.func = copy.deepcopy(transform)
        self.stats = copy.deepcopy(stats)
        self.field = copy.deepcopy(field)
        self.z = copy.deepcopy(z)

    def __call__(self, x, field=None, z=None):
        return self.func(x, self.field if field is None else field, self.z if z is None else z, self.stats)


def compile_transform(transform, stats={}, field=None, z=None):
    return _Compiled(transform, stats, field, z)


class _TileDatasetBase:
    """What the painter reads from a dataset (painter.py:114-116,307,321,399-412)."""

    def create_transform(self, field, z):
        return compile_transform(self.transform_func, self.stats, field, z)

    def create_inverse_transform(self, field, z):
        return compile_transform(self.inverse_transform_func, self.stats, field, z)

    def _field_list(self):
        return [self.input_field] + self.label_fields

    def get_transforms(self, idx=None, z=None):
        if idx is None and z is None:
            raise ValueError("Either idx or z have to be specified.")
        z = self.sample_idx_to_redshift(idx) if z is None else z
        return [self.create_transform(f, z) for f in self._field_list()]

    def get_inverse_transforms(self, idx=None, z=None):
        if idx is None and z is None:
            raise ValueError("Either idx or z have to be specified.")
        z = self.sample_idx_to_redshift(idx) if z is None else z
        return [self.create_inverse_transform(f, z) for f in self._field_list()]

    def sample_idx_to_redshift(self, idx):
        return self.redshifts[idx // self.n_sample]

    def __len__(self):
        return self.n_sample * len(self.redshifts)

    def get_batch(self, size=1, z=None, idx=None):
        """Random batch: (fields (1+F, N, C, H, W), indices, redshifts) -- datasets.py:434-473."""
        if idx is None:
            idx = np.random.choice(self.n_sample, size=size, replace=False)
            if z is None:
                idx *= len(self.redshifts)            # sic (datasets.py:459)
                z = [self.sample_idx_to_redshift(i) for i in idx]
            else:
                idx += self.redshifts.index(z) * self.n_sample
                z = [z] * size
        else:
            z = [self.sample_idx_to_redshift(i) for i in idx]
        samples = [self[i][0] for i in idx]
        return np.array(samples).swapaxes(0, 1), idx, np.array(z)


class BAHAMASDataset(_TileDatasetBase):
    def __init__(self, data=None, files=None, root_path=None, redshifts=[], input_field="dm", label_fields=[],
                 n_tile=4, L=400, n_stack=None, stack_offset=0, transform=_identity, inverse_transform=_identity,
                 n_feature_per_field=1, tile_permutations=False, scale_to_SLICS=True, subtract_minimum=False,
                 mmap_mode="r", verbose=False, fixed_indexing=False):
        fields, zs = [], []
        if data is not None:
            self.data = data
            fields = list(data.keys())
            zs = list(data[fields[0]].keys())
        elif files is not None:
            self.data = {}
            for f in files:
                if not isinstance(f, dict):
                    raise ValueError("files entry is not a dict.")
                fields.append(f["field"])
                zs.append(f["z"])
        else:
            raise ValueError("Either data or files need to be provided.")
        self.fields = list(collections.OrderedDict.fromkeys(fields))
        self.redshifts = list(collections.OrderedDict.fromkeys(zs))
        self.input_field = input_field
        if label_fields != []:
            self.label_fields = label_fields
            missing = set([input_field] + label_fields) - set(self.fields)
            if missing:
                raise ValueError(f"The requested fields are not in the file list: field(s) {missing} is missing.")
            self.fields = [input_field] + label_fields
        else:
            self.label_fields = [f for f in self.fields if f != input_field]
        if redshifts != []:
            missing = set(redshifts) - set(self.redshifts)
            if missing:
                raise ValueError(f"The requested redshifts are not in the file list: redshift(s) {missing} is missing.")
            self.redshifts = redshifts
        else:
            self.redshifts = sorted(self.redshifts)

        if files is not None:
            for f in files:
                field, z = f["field"], f["z"]
                if field not in self.fields or z not in self.redshifts:
                    continue
                entry = self.data.setdefault(field, {}).setdefault(z, {})
                for slab in ("100", "150"):
                    fn = f["file_" + slab]
                    if root_path is not None:
                        fn = os.path.join(root_path, fn)
                    entry[slab] = np.load(fn, mmap_mode=mmap_mode)
                    entry["mean_" + slab] = f["mean_" + slab]
                    entry["var_" + slab] = f["var_" + slab]

        first = self.data[self.fields[0]][self.redshifts[0]]
        self.n_stack_100, self.n_grid, _ = first["100"].shape
        self.n_stack_150 = first["150"].shape[0]
        self.n_stack = min(self.n_stack_100, self.n_stack_150) if n_stack is None else n_stack
        self.stack_offset = stack_offset
        if min(self.n_stack_100, self.n_stack_150) < self.stack_offset + self.n_stack:
            raise ValueError("Highest stack exceeds number of available stacks.")
        self.n_tile_permutation = 8 if tile_permutations else 1
        self.n_tile = n_tile
        self.tile_size = self.n_grid // n_tile
        self.n_total_sample = ((self.n_stack_100 * n_tile ** 2 * self.n_tile_permutation)
                               * (self.n_stack_150 * n_tile ** 2 * self.n_tile_permutation))
        self.n_sample = self.n_stack ** 2 * n_tile ** 4 * self.n_tile_permutation ** 2
        self.L = L
        self.tile_L = L / n_tile
        self.transform_func, self.inverse_transform_func = transform, inverse_transform
        self.n_feature_per_field = n_feature_per_field
        self.scale_to_SLICS, self.subtract_minimum = scale_to_SLICS, subtract_minimum
        self.fixed_indexing = fixed_indexing
        self.stats = collections.OrderedDict()
        for field in self.fields:
            self.stats[field] = collections.OrderedDict((z, self.get_stack_stats(field, z)) for z in self.redshifts)
        self.transform = compile_transform(transform, self.stats)
        self.inverse_transform = compile_transform(inverse_transform, self.stats)

    def get_stack_stats(self, field, z):
        d = self.data[field][z]
        stats = {"mean": d["mean_100"] + d["mean_150"], "var": d["var_100"] + d["var_150"]}
        if field == self.input_field and self.scale_to_SLICS:
            s = slics_scale(self.n_grid)
            stats["mean"] *= s
            stats["var"] *= s ** 2
        return stats

    # ---- the index arithmetic (pure integers)
    def sample_idx_to_tile_permutation(self, idx):
        sample_idx = idx % self.n_sample
        p = sample_idx // (self.n_sample // self.n_tile_permutation ** 2)
        return tuple(int(v) for v in np.unravel_index(p, (self.n_tile_permutation,) * 2))

    def sample_idx_to_tile(self, flat_idx):
        """-> (stack_100, ty_100, tx_100, stack_150, ty_150, tx_150) of a flat sample index."""
        no_z = flat_idx % self.n_sample
        if self.fixed_indexing:
            base = no_z % (self.n_sample // self.n_tile_permutation ** 2)
        else:
            base = no_z % self.n_tile_permutation ** 2          # sic (datasets.py:327)
        i = np.unravel_index(base, (self.n_stack, self.n_tile, self.n_tile) * 2)
        i = [int(v) for v in i]
        return (i[0] + self.stack_offset, i[1], i[2], i[3] + self.stack_offset, i[4], i[5])

    def apply_tile_permutation(self, tile, permutation_idx):
        rot, flip = permutation_idx // 4, permutation_idx % 4
        if rot > 0:
            tile = np.rot90(tile, k=rot)
        if flip == 1:
            tile = tile[:, ::-1]
        elif flip == 2:
            tile = tile[::-1]
        elif flip == 3 and self.fixed_indexing:
            tile = tile[::-1, ::-1]                               # unreachable in the reference
        return tile

    def get_stack(self, field, z, flat_idx):
        s100, y100, x100, s150, y150, x150 = self.sample_idx_to_tile(flat_idx)
        t = self.tile_size
        d100 = self.data[field][z]["100"][s100][y100 * t:(y100 + 1) * t, x100 * t:(x100 + 1) * t]
        d150 = self.data[field][z]["150"][s150][y150 * t:(y150 + 1) * t, x150 * t:(x150 + 1) * t]
        p100, p150 = self.sample_idx_to_tile_permutation(flat_idx)
        return self.apply_tile_permutation(d100, p100) + self.apply_tile_permutation(d150, p150)

    def get_input_sample(self, idx, transform=True):
        z = self.sample_idx_to_redshift(idx)
        d = self.get_stack(self.input_field, z, idx)
        if self.scale_to_SLICS:
            d = slics_scale(self.n_grid) * d
        if self.subtract_minimum:
            d = d - d.min()
        return self.transform(d, self.input_field, z) if transform else d

    def get_label_sample(self, idx, transform=True):
        z = self.sample_idx_to_redshift(idx)
        out = []
        for f in self.label_fields:
            d = self.get_stack(f, z, idx)
            out.append(self.transform(d, f, z) if transform else d)
        return out

    def __getitem__(self, idx):
        if isinstance(idx, collections.abc.Iterable):
            raise NotImplementedError("Only int indicies are supported for now.")
        return [self.get_input_sample(idx)] + self.get_label_sample(idx), idx, self.sample_idx_to_redshift(idx)


class SyntheticTileDataset(_TileDatasetBase):
    """Seeded synthetic (dm, pressure) tiles in the transformed domain, same protocol as
    ``BAHAMASDataset``; sample ``i`` is a pure function of ``(seed, i)``."""

    def __init__(self, n_sample=256, tile_size=512, redshifts=syn.REDSHIFTS, seed=0, L=400, n_tile=4):
        self.n_sample = n_sample
        self.redshifts = list(redshifts)
        self.tile_size = tile_size
        self.seed = seed
        self.input_field, self.label_fields = "dm", ["pressure"]
        self.fields = ["dm", "pressure"]
        self.n_feature_per_field = 1
        self.L, self.n_tile = L, n_tile
        self.n_grid = tile_size * n_tile
        self.tile_L = L / n_tile
        self.scale_to_SLICS = False
        self.stats = collections.OrderedDict()
        for f in self.fields:
            self.stats[f] = collections.OrderedDict(
                (z, {"mean": 1.0, "var": syn.field_sigma(f, z) ** 2}) for z in self.redshifts)
        from . import data_transforms as T
        fwd, inv = T.create_range_compress_transforms({"dm": 4.0, "pressure": 4}, {"dm": "shift-log",
                                                                                  "pressure": "shift-log"})
        self.transform_func = T.chain_transformations([fwd, T.atleast_3d, T.as_float32])
        self.inverse_transform_func = T.chain_transformations([T.squeeze, inv])
        self.transform = compile_transform(self.transform_func, self.stats)
        self.inverse_transform = compile_transform(self.inverse_transform_func, self.stats)

    def raw_fields(self, idx):
        z = self.sample_idx_to_redshift(idx)
        rng = np.random.Generator(np.random.PCG64([self.seed, idx]))
        t = self.tile_size
        g = np.sqrt(-2 * np.log(1 - rng.random((t, t)))) * np.cos(2 * np.pi * rng.random((t, t)))
        g2 = np.sqrt(-2 * np.log(1 - rng.random((t, t)))) * np.cos(2 * np.pi * rng.random((t, t)))
        dm = (np.exp(0.9 * g - 0.4) * syn.field_sigma("dm", z)).astype(np.float32)
        pr = (0.05 * np.exp(0.8 * g + 0.6 * g2 - 0.5) * syn.field_sigma("pressure", z) / 0.05).astype(np.float32)
        return dm, pr, z

    def __getitem__(self, idx):
        if isinstance(idx, collections.abc.Iterable):
            raise NotImplementedError("Only int indicies are supported for now.")
        dm, pr, z = self.raw_fields(int(idx))
        return [self.transform(dm, "dm", z), self.transform(pr, "pressure", z)], idx, z


class DeviceTileAssembler:
    """Batch assembly on the GPU for a ``BAHAMASDataset``: the stacks are uploaded to HBM once
    (fiducial training set: 2 fields x 11 redshifts x 2 slabs x 14 x 2048^2 floats = 10 GB of the
    288 GB) and every batch is one gather launch per field that reads the two tiles of each sample,
    applies the tile permutation, adds them, scales and transforms them -- bit-for-bit the index
    arithmetic of ``BAHAMASDataset.get_stack`` (computed on the host, integers only), so 8 GPUs are not
    starved by a serial ``DataLoader(num_workers=0)`` (painter.py:88).

    The transform comes from the dataset's chain (``dataset.transform_func``), read by the functions the paint path
    uses (``data_transforms.device_shift_log`` / ``device_split_scale``): the identity, ONE range compression (any of
    the six modes, one per field) among shape-only steps, or ``[range compression, as_float32 (optional), split-scale,
    shape-only steps ...]``, for which every field of a sample comes out as its ``levels`` pyramid planes
    (``bp_gather_tiles_scales``: the gather runs inside the first filter pass).  A "shift-log" field goes through the
    entry points it always went through; a field of another mode through ``bp_gather_tiles_scales_mode`` with the
    records of ``DeviceRangeCompress.records``.  Any other chain raises NotImplementedError in the constructor, before a
    stack is uploaded.  ``subtract_minimum`` datasets are served by a per-tile minimum on the device (``bp_tile_minima``),
    subtracted in float32 in front of the transform, bit-equal to the host's ``d - d.min()``.  ``k_values`` (with
    ``mode="shift-log"``) or ``mode=None`` given explicitly mean a single-scale batch without reading the chain."""

    REC100 = np.dtype([("base", np.int64), ("pitch", np.int32), ("r0", np.int32), ("rr", np.int32),
                       ("rc", np.int32), ("c0", np.int32), ("cr", np.int32), ("cc", np.int32), ("pad", np.int32)])
    XF = np.dtype([("scale", np.float64), ("inv_sigma", np.float64), ("inv_k", np.float64),
                   ("mode", np.int32), ("pad", np.int32)])

    def __init__(self, dataset, device="cuda:0", k_values=None, mode="shift-log"):
        import torch
        from .. import _lib as L
        from . import data_transforms as T
        self.ds, self.device, self.torch, self.L = dataset, torch.device(device), torch, L
        self.lib = L.load()
        if mode not in ("shift-log", None):
            raise NotImplementedError("an explicit mode is 'shift-log' or None; the other range-compression modes are "
                                      "read from the dataset's chain (k_values=None)")
        self.scales = None
        self.compress = {}                               # field -> DeviceRangeCompress of a mode other than shift-log
        if k_values is None and mode == "shift-log":
            found, self.scales = self._read_compressions(dataset, T)
            mode, k_values = ("shift-log" if found else None), {f: float(rc) for f, rc in found.items()}
            self.compress = {f: rc for f, rc in found.items() if rc.name != "shift-log"}
        self.mode = mode
        self.k_values = k_values or {}
        self._interp = T.interpolate_z
        self._scratch = None                             # the pyramid's planes, grown to the largest batch
        if self.scales is not None:                      # the pyramid's tables go up once per assembler
            sc = self.scales
            radii, weights = T.split_scale_tables(sc["n_scale"], sc["step_size"], sc["truncate"])
            sc["radii"] = (C.c_int32 * len(radii))(*radii)
            sc["weights"] = torch.from_numpy(weights).to(self.device) if sc["n_scale"] > 1 else None
        self.stacks = {}
        for f in dataset.fields:
            for z in dataset.redshifts:
                for slab in ("100", "150"):
                    a = np.ascontiguousarray(dataset.data[f][z][slab], dtype=np.float32)
                    self.stacks[(f, z, slab)] = torch.from_numpy(a).to(self.device)

    @staticmethod
    def _read_compressions(dataset, T):
        """({field: DeviceRangeCompress}, scales) of ``dataset.transform_func`` ({} for the identity);
        NotImplementedError for a chain without a device form, and for a forward chain whose mode of a field is not the
        one the range compression of ``dataset.inverse_transform_func`` (if it has one) undoes."""
        func, fields = dataset.transform_func, [dataset.input_field] + list(dataset.label_fields)
        if func is _identity or func is None:
            return {}, None
        scales = None
        if T.has_split_scale(func):
            found = [T.device_split_scale(func, 0, f) for f in fields]
            split = found[0][1]
            scales = {"n_scale": split.n_scale, "step_size": split.step_size,
                      "include_original": bool(split.include_original), "truncate": split.truncate}
            found = {f: rc for f, (rc, _) in zip(fields, found)}
        else:
            found = {f: T.device_shift_log(func, 0, f) for f in fields}
        # The mode is now read per field, so it is checked against the range compression the dataset's inverse chain
        # undoes, where that chain holds one: a set whose two chains name different modes for a field would train on
        # tiles that the transforms its checkpoints carry do not invert.
        for st in T.chain_steps(getattr(dataset, "inverse_transform_func", None)):
            if isinstance(st, T._RangeCompress) and st.direction == 1:
                for f, rc in found.items():
                    if str(st.modes.get(f, rc.name)).lower() != rc.name:
                        raise NotImplementedError(
                            f"field '{f}' is compressed with '{rc.name}' but the dataset's inverse transform undoes "
                            f"'{st.modes[f]}': such a pair of chains has no device form")
        return found, scales

    @classmethod
    def _read_chain(cls, dataset, T):
        """(mode, k_values, scales) of ``dataset.transform_func``: mode "shift-log" (None for the identity), or
        {field: mode name} where a field has another mode; NotImplementedError for a chain without a device form."""
        found, scales = cls._read_compressions(dataset, T)
        if not found:
            return None, {}, scales
        names = {f: rc.name for f, rc in found.items()}
        mode = "shift-log" if set(names.values()) == {"shift-log"} else names
        return mode, {f: (rc.k[0] if len(rc.k) == 1 else tuple(rc.k)) for f, rc in found.items()}, scales

    @property
    def levels(self):
        """Channels per field of a batch."""
        return 1 if self.scales is None else self.scales["n_scale"] + int(self.scales["include_original"])

    def _perm_affine(self, p):
        """``_perm_affine_compute(p)``, computed once per assembler and code: the two t x t index grids it builds cost more
        than a training step at 512^2 when every sample asks for them four times."""
        memo = self.__dict__.setdefault("_affine_memo", {})
        key = (self.ds.tile_size, int(p))
        if key not in memo:
            memo[key] = self._perm_affine_compute(p)
        return memo[key]

    def _perm_affine_compute(self, p):
        """(r0, rr, rc, c0, cr, cc) of ``apply_tile_permutation`` for code p, from the images of three
        index points under the very same NumPy operations."""
        t = self.ds.tile_size
        rows, cols = np.meshgrid(np.arange(t), np.arange(t), indexing="ij")
        pr = self.ds.apply_tile_permutation(rows, p)
        pc = self.ds.apply_tile_permutation(cols, p)
        r0, c0 = int(pr[0, 0]), int(pc[0, 0])
        return (r0, int(pr[1, 0]) - r0, int(pr[0, 1]) - r0, c0, int(pc[1, 0]) - c0, int(pc[0, 1]) - c0)

    def _descriptors(self, field, indices):
        ds, t = self.ds, self.ds.tile_size
        d100 = np.zeros(len(indices), self.REC100)
        d150 = np.zeros(len(indices), self.REC100)
        xf = np.zeros(len(indices), self.XF)
        for n, idx in enumerate(indices):
            idx = int(idx)
            z = ds.sample_idx_to_redshift(idx)
            s100, y100, x100, s150, y150, x150 = ds.sample_idx_to_tile(idx)
            p100, p150 = ds.sample_idx_to_tile_permutation(idx)
            for rec, slab, s, ty, tx, p in ((d100, "100", s100, y100, x100, p100), (d150, "150", s150, y150, x150, p150)):
                st = self.stacks[(field, z, slab)]
                g = st.shape[-1]
                rec[n]["base"] = st.data_ptr() + 4 * ((s * g + ty * t) * g + tx * t)
                rec[n]["pitch"] = g
                (rec[n]["r0"], rec[n]["rr"], rec[n]["rc"], rec[n]["c0"], rec[n]["cr"], rec[n]["cc"]) = self._perm_affine(p)
            scale = slics_scale(ds.n_grid) if (field == ds.input_field and ds.scale_to_SLICS) else 1.0
            xf[n]["scale"] = scale
            if self.mode == "shift-log" and field not in self.compress:
                sig = np.sqrt(self._interp(ds.stats[field], z)["var"])
                xf[n]["inv_sigma"] = 1.0 / sig
                xf[n]["inv_k"] = 1.0 / float(self.k_values[field])
                xf[n]["mode"] = 1
        return d100, d150, xf

    def get_batch(self, indices):
        """-> (x = label field(s) (N,F*levels,t,t), y = input field (N,levels,t,t), aux = redshift (N,)) on the device;
        levels = 1 for a single-scale dataset."""
        torch, L, ds, t = self.torch, self.L, self.ds, self.ds.tile_size
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        n, levels = len(indices), self.levels
        sc = self.scales or {"n_scale": 1, "include_original": False, "weights": None, "radii": None}
        outs, keep = [], []
        for field in [ds.input_field] + ds.label_fields:
            d100, d150, xf = self._descriptors(field, indices)
            dev = [torch.from_numpy(a.view(np.uint8)).to(self.device) for a in (d100, d150, xf)]
            keep.append(dev)
            out = torch.empty((n, levels, t, t), device=self.device)
            minima = None
            if ds.subtract_minimum and field == ds.input_field:      # datasets.py:398-403: the input field only
                minima = torch.empty(n, device=self.device)
                keep.append(minima)
                L.check(self.lib.bp_tile_minima(L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]), n, t, L.ptr(minima), st),
                        "tile minima")
            rc = self.compress.get(field)
            records = None
            if rc is not None:                                       # a mode other than shift-log: its (n, 4) records
                zs = [ds.sample_idx_to_redshift(int(i)) for i in indices]
                records = torch.from_numpy(rc.records(ds.stats[field], zs)).to(self.device)
                keep.append(records)
            if self.scales is None and minima is None and rc is None:
                L.check(self.lib.bp_gather_tiles(L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]), n, t, L.ptr(out), st),
                        "gather tiles")
            else:
                ws = int(self.lib.bp_gather_tiles_scales_workspace(n, t, sc["n_scale"]))
                if ws and (self._scratch is None or self._scratch.numel() < ws):
                    self._scratch = torch.empty(ws, dtype=torch.uint8, device=self.device)
                args = (L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]), L.ptr(minima), n, t, sc["n_scale"],
                        int(sc["include_original"]), L.ptr(sc["weights"]), sc["radii"],
                        L.ptr(self._scratch if ws else None), ws, L.ptr(out), st)
                if rc is None:
                    L.check(self.lib.bp_gather_tiles_scales(*args), "gather tiles into scales")
                else:
                    L.check(self.lib.bp_gather_tiles_scales_mode(rc.mode, L.ptr(records), *args),
                            f"gather tiles into scales ({rc.name})")
            outs.append(out)
        torch.cuda.current_stream().synchronize()        # descriptors may be freed after this
        z = torch.tensor([ds.sample_idx_to_redshift(int(i)) for i in indices], device=self.device,
                         dtype=torch.float32)
        return torch.cat(outs[1:], dim=1), outs[0], z

    def _gan_block(self, indices, cam, aux):
        """The packed host image of one ``bp_gather_tiles_gan`` call: {name: (byte offset, array)} and its size.  The tile
        descriptors of both fields (those of ``_descriptors``, with the index arithmetic done once per sample), the two
        scale records, ``cam`` (n, 2, 3) float64 and ``aux`` (n,) float32, every part 8-byte aligned."""
        ds, t = self.ds, self.ds.tile_size
        fields = (ds.input_field, ds.label_fields[0])
        rows = {(f, slab): [] for f in fields for slab in ("100", "150")}
        for idx in indices:
            idx = int(idx)
            z = ds.sample_idx_to_redshift(idx)
            s100, y100, x100, s150, y150, x150 = ds.sample_idx_to_tile(idx)
            p100, p150 = ds.sample_idx_to_tile_permutation(idx)
            for slab, s, ty, tx, p in (("100", s100, y100, x100, p100), ("150", s150, y150, x150, p150)):
                aff = self._perm_affine(p)
                for f in fields:
                    st = self.stacks[(f, z, slab)]
                    g = st.shape[-1]
                    rows[(f, slab)].append((st.data_ptr() + 4 * ((s * g + ty * t) * g + tx * t), g) + aff + (0,))
        n = len(indices)
        xf = {f: np.zeros(n, self.XF) for f in fields}
        xf[fields[0]]["scale"] = slics_scale(ds.n_grid) if ds.scale_to_SLICS else 1.0
        xf[fields[1]]["scale"] = 1.0
        cam = np.ascontiguousarray(cam, dtype=np.float64)
        aux = np.ascontiguousarray(aux, dtype=np.float32)
        if cam.shape != (n, 2, 3) or aux.shape != (n,):
            raise ValueError(f"cam {cam.shape} / aux {aux.shape}: expected ({n}, 2, 3) and ({n},)")
        parts = [("in100", np.array(rows[(fields[0], "100")], self.REC100)),
                 ("in150", np.array(rows[(fields[0], "150")], self.REC100)), ("in_xf", xf[fields[0]]),
                 ("lab100", np.array(rows[(fields[1], "100")], self.REC100)),
                 ("lab150", np.array(rows[(fields[1], "150")], self.REC100)), ("lab_xf", xf[fields[1]]),
                 ("cam", cam), ("aux", aux)]
        layout, off = {}, 0
        for name, a in parts:
            layout[name] = (off, a)
            off += (a.nbytes + 7) // 8 * 8
        return layout, off

    def gather_gan(self, indices, cam, aux, plan):
        """One CGAN training batch, written straight into the inputs of the training plan ``plan`` (models.cgan._GanPlan of
        ``len(indices)`` samples) by ONE ``bp_gather_tiles_gan`` launch on the current stream: the generator's input, both
        halves' conditioning channels and the real field of the discriminator's input, and the dense label plane.

        ``cam``: (n, 2, 3) float64, {sigma, k0, k1} of the input field and of the label field per sample (the CGAN's
        "shift-log-cam" transform); ``aux``: (n,) float32, the conditioning value.  The assembler is one built with
        ``mode=None``: no chain is read, of the scale records only ``scale`` is used.  ``subtract_minimum`` sets get the
        input field's ``bp_tile_minima`` in front.  Descriptors, ``cam`` and ``aux`` go up as one packed block in one
        host-to-device copy from pinned memory; nothing waits for the device: the block (and the minima) are stream-ordered
        memory of the caching allocator and may be released as soon as the launches are enqueued."""
        torch, L, ds, t = self.torch, self.L, self.ds, self.ds.tile_size
        n = len(indices)
        if plan.n != n:
            raise ValueError(f"the plan holds {plan.n} samples, the batch {n}")
        layout, nbytes = self._gan_block(indices, cam, aux)
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)     # (the caching host allocator keeps it until
        hv = host.numpy()                                                  # the copy below has run)
        for off, a in layout.values():
            hv[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        dev = host.to(self.device, non_blocking=True)
        base = dev.data_ptr()
        p = {name: C.c_void_p(base + off) for name, (off, _) in layout.items()}
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        minima = None
        if ds.subtract_minimum:
            minima = torch.empty(n, device=self.device)
            L.check(self.lib.bp_tile_minima(p["in100"], p["in150"], p["in_xf"], n, t, L.ptr(minima), st), "tile minima")

        def fill(gen_in, d_real, d_fake_cond, x_nchw):
            L.check(self.lib.bp_gather_tiles_gan(p["in100"], p["in150"], p["in_xf"], L.ptr(minima), p["lab100"],
                                                 p["lab150"], p["lab_xf"], p["cam"], p["aux"], n, t, C.byref(gen_in),
                                                 C.byref(d_real), C.byref(d_fake_cond), L.ptr(x_nchw), st),
                    "gather tiles (CGAN)")
        plan.fill(fill)
