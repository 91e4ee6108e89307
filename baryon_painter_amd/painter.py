"""Painter API: train / validate / paint / checkpoint, with the reference's signatures.

Mirrors ``baryon_painter.painter`` (/root/reference/baryon_painter/painter.py:16-545).  The loop
semantics that affect results are kept: pseudo-epoch bookkeeping (one ``scheduler.step()`` per
pseudo epoch, painter.py:179-190), adaptive batch size by rebuilding the DataLoader
(:210-215), validation losses computed under ``no_grad`` but in TRAIN mode (:85,306-314 -- they
update batch-norm running statistics, as in the reference), ``paint`` switching to eval mode
for good (:372), file names and the text format of the statistics logs (:127-131,476-484).
Out of scope and therefore absent: the matplotlib / cosmotools diagnostics
(``validation_plotting``); ``show_plots`` / ``save_plots`` / ``plot_*`` arguments are accepted
and ignored, and the two reference crashes they trigger do not occur.
"""
import collections
import os
import pickle

import numpy as np
import torch
import torch.utils.data

from .models import cvae as _cvae
from .models import paint_graph as PG
from .models.paint_graph import seed_word as _seed_word      # noqa: F401  (the name this module had for it)
from .utils import datasets

try:                                    # the reference pickles its metadata with dill
    import dill as _pickler
except ImportError:                     # pragma: no cover
    _pickler = pickle


SCORE_KEYS = ("bound", "elbo", "log_likelihood", "kl", "ess")      # the columns of ``CVAE.score``, in order


class Painter:
    """Abstract base class for a baryon painter (painter.py:16-31)."""

    def __init__(self):
        raise NotImplementedError("This is an abstract base class.")

    def load_state_from_file(self, filename):
        raise NotImplementedError("This is an abstract base class.")

    def paint(self, input, **kwargs):
        raise NotImplementedError("This is an abstract base class.")

    # ---- device paint paths, shared by the painters whose model has a ``paint_graph`` (CVAEPainter, CGANPainter).  A
    # painter supplies ``_tile_shape()`` -> (H, W), ``_shape_mismatch(shape)`` -> the message for tiles of another shape,
    # and ``_device_paint_parameters(zs)`` -> (params, scales, modes) of ``_paint_stream_pipeline`` for tiles at
    # redshifts ``zs``, NotImplementedError where the painter has no device form (raised before any capture).
    def release_paint_buffers(self):
        """Free what the device paint paths keep between calls: ``paint_stream``'s page-locked host staging buffers -- two
        parameter blocks plus up to four (batch, 1, H, W) fp32 buffers, 256 MiB of pinned memory at batch 64 of 512^2
        tiles ((batch, F, H, W) on the output side of a painter with F label fields), which otherwise live as long as the
        painter (page-locking them costs tens of milliseconds per call, hence the cache) -- and
        ``_paint_plane_device``'s accumulators and scratch, the K accumulator pairs of a plane ensemble included."""
        self.__dict__.pop("_paint_host_buffers", None)
        self.__dict__.pop("_plane_device_buffers", None)

    def _need_pixel_noise(self):
        """ValueError unless this painter can paint draws from its likelihood (``pixel_noise=True``): a CVAE with a
        variance head.  No side effects: nothing is captured, no random number is drawn."""
        raise ValueError(f"pixel_noise=True: {type(self).__name__} has no likelihood with a variance head to draw from")

    def _stream_prologue(self, inputs, z, tile_ids, rank, world_size):
        """What ``paint_stream`` and ``paint_ensemble`` begin with: the model in eval mode, the tiles' shape checked
        (ValueError), ``z`` broadcast over the N tiles, ``tile_ids`` defaulting to 0 ... N - 1, and this rank's share
        [lo, hi) of the tiles.  Returns (model, (H, W), N, zs, ids, lo, hi); nothing is captured."""
        model = self.model
        model.train(False)
        H, W = self._tile_shape()
        N = len(inputs)
        if tuple(inputs.shape[1:]) != (H, W):
            raise ValueError(self._shape_mismatch(tuple(inputs.shape)))
        zs = np.broadcast_to(np.asarray(z, dtype=np.float64), (N,))
        ids = np.arange(N, dtype=np.int64) if tile_ids is None else np.asarray(tile_ids, dtype=np.int64)
        per = (N + world_size - 1) // world_size
        return model, (H, W), N, zs, ids, min(rank * per, N), min((rank + 1) * per, N)

    def paint_stream(self, inputs, z, batch_size=64, tile_ids=None, seed=0, rank=0, world_size=1, out=None,
                     pixel_noise=False, noise_ids=None, noise_origins=None):
        """Paint MANY raw tiles: ``inputs`` (N, H, W) float32 host array (NumPy, memory map, or a pinned torch tensor),
        redshifts ``z`` (scalar or (N,)) -> (N, H, W) float32 physical tiles.  The production form of ``paint``
        (process_SLICS.py:201-218 calls it tile by tile):

          * the transform and its inverse run on the device, fused into the layout kernels on either side of the
            network (``bp_paint_load`` / ``bp_paint_store`` and their kin), bit-compatible with the host transforms;
          * batches of ``batch_size`` tiles replay ONE captured hipGraph (``model.paint_graph``);
          * host->device and device->host copies go through pinned double buffers on their own streams, so that
            batch b+1 is uploaded and batch b-1 downloaded while batch b is painted;
          * a CVAE's prior noise of tile i comes from a counter-based generator keyed on (``seed``, ``tile_ids[i]``
            [default: i], int64), so the result does not depend on ``batch_size`` or on how tiles are dealt to ranks;
            the seed travels in the per-batch parameter block: one captured graph serves every seed;
          * ``rank`` / ``world_size``: this process paints the contiguous block of tiles that is its share (one
            process per GPU, no collective: tiles are independent) and returns (block, (lo, hi));
          * a CVAE painter with F > 1 label fields returns (N, F, H, W): field j from head channels
            [j * nf, (j + 1) * nf) through ``label_fields[j]``'s inverse, all fields stored by one launch
            (``bp_paint_store_fields``); ``out``, where given, has that shape;
          * ``pixel_noise=True`` (a CVAE painter with a variance head; ValueError otherwise, before any capture): every
            tile is a DRAW from the likelihood, x_mu + sqrt(x_var) e in network units in front of the inverse
            transform, not its mean.  e of tile i is a window of a noise lattice (``bp_likelihood_draw``) under the key
            ``seed``: lattice ``noise_ids[i]`` [default: ``tile_ids[i]``], window origin ``noise_origins[i]`` =
            (row, col) >= 0 [default: (0, 0)].  Like the latent noise it does not depend on batches or ranks; tiles that
            share an id see the same e where their windows overlap."""
        model, (H, W), N, zs, ids, lo, hi = self._stream_prologue(inputs, z, tile_ids, rank, world_size)
        if pixel_noise:
            self._need_pixel_noise()
        params, scales, modes = self._device_paint_parameters(zs[lo:hi])     # (NotImplementedError before any capture)
        if pixel_noise:
            params = _with_noise(params, ids if noise_ids is None else noise_ids, noise_origins, N, H, W, lo, hi)
        result = _paint_stream_pipeline(self, model, inputs, (H, W), lo, hi, int(batch_size), params, ids[lo:hi], seed,
                                        out, scales, modes)
        return (result, (lo, hi)) if world_size > 1 else result

    def _ensemble_parameters(self, zs, pixel_noise):
        """``_device_paint_parameters(zs, ensemble=True)`` for the plane ensembles: NotImplementedError for a painter
        without ``paint_ensemble`` (no latent to draw from) and for ``pixel_noise``.  No side effects."""
        if not hasattr(self, "paint_ensemble"):
            raise NotImplementedError(f"{type(self).__name__} has no latent to draw an ensemble from")
        if pixel_noise:
            raise NotImplementedError("an ensemble of planes has no pixel noise: an ensemble block has no noise_org, so "
                                      "overlapping tiles could not share their noise lattice")
        return self._device_paint_parameters(zs, ensemble=True)

    def _paint_plane_device(self, delta, geo, z, weight_map, batch_size, tile_ids, seed, regularise_std=None, out=None,
                            pixel_noise=False, draws=None, return_planes=False, moments=True, regularise=True,
                            keep=None):
        """The device form of ``lightcone.paint_plane`` (on_device=True): ``geo`` is ``lightcone.plane_geometry``'s,
        ``weight_map`` the host's ``make_weight_map`` (float64, uploaded as it is), ``tile_ids`` / ``seed`` / ``batch_size``
        those the host path hands to ``paint_stream``.  Per batch, on ONE stream: the tiles are cut (and resampled) from
        the device plane into a slot's ``raw`` (bp_plane_cut), the batch's parameter block is copied in from a per-plane
        device copy, the graph is replayed, and the slot's ``out`` is blended into float64 accumulators
        (bp_plane_blend); bp_plane_finish divides.  Returns the (n_plane, n_plane) float64 plane, or ``out`` (a CUDA
        float64 tensor of that shape) filled in place.  A painter with F > 1 label fields blends its (B, F, tile, tile)
        ``out`` with bp_plane_blend_fields, each field into a plane of its own with its own regularisation mask: the
        plane, and ``out``, is (F, n_plane, n_plane).  ``pixel_noise``: as on the host path, every tile draws from the
        lattice ``tile_ids[0]`` at its destination origin ``geo["dst"]``.

        ``draws`` = K (``lightcone.paint_plane_ensemble``; a painter with ``paint_ensemble``, NotImplementedError
        otherwise and with ``pixel_noise``; ``batch_size`` then counts TILES per batch): every draw is blended into a
        plane of its own and the moments are taken across the K planes (``_paint_plane_ensemble_pipeline``).  Returns
        (mean, var), with ``return_planes`` (mean, var, planes), planes (K, [F,] n_plane, n_plane); ``out`` is the pair
        (mean, var) of CUDA float64 tensors.  ``moments=False``: the K finished planes alone, as a CUDA tensor that
        lives in the cached accumulator until the next plane is painted.  Without ``draws`` nothing changes.

        ``regularise=False`` (single draws only): the blend is not masked, whatever ``regularise_std`` says.  ``keep``: a
        ``TileKeep.plane(...)`` record -- each batch's tiles are counted (bp_tile_outliers) and its problematic tiles
        set aside (bp_tile_keep) between the replay and the blend; without it the plane's launches are unchanged."""
        model = self.model
        model.train(False)
        tile, W = self._tile_shape()
        if tile != W:
            raise NotImplementedError("device planes need square tiles")
        if tuple(weight_map.shape) != (tile, tile):
            raise ValueError(f"weight map {weight_map.shape} does not match the model's {tile}^2 tiles")
        if draws is not None and (keep is not None or not regularise):
            raise NotImplementedError("plane ensembles have no tile report and no detect-only mode")
        if draws is not None:
            K = PG.check_draws(draws)
            params, scales, modes = self._ensemble_parameters(np.full(len(geo["origins"]), float(z)), pixel_noise)
            return _paint_plane_ensemble_pipeline(self, model, tile, delta, geo, int(batch_size), K, params, tile_ids, seed,
                                                  weight_map, regularise_std, out, scales, modes, return_planes, moments)
        if pixel_noise:
            self._need_pixel_noise()
        params, scales, modes = self._device_paint_parameters(np.full(len(geo["origins"]), float(z)))
        if pixel_noise:
            # one lattice per plane, each tile's window at its place in the painted plane: where tiles overlap they
            # carry the same noise, and the feathered blend does not average it away (lightcone.paint_plane)
            n = len(geo["origins"])
            params = _with_noise(params, np.full(n, tile_ids[0], dtype=np.int64), geo["dst"], n, tile, tile, 0, n)
        return _paint_plane_pipeline(self, model, tile, delta, geo, int(batch_size), params, tile_ids, seed, weight_map,
                                     regularise_std if regularise else None, out, scales, modes, keep)

    def _paint_small_plane_device(self, plane, origin, size, crop, z, tile_id, seed, subtract_minimum=False,
                                  field_index=None, out=None, pixel_noise=False, draws=None, return_planes=False,
                                  moments=True):
        """The device form of ``lightcone.paint_small_plane`` (on_device=True), on ONE stream and without a host
        synchronisation: ``plane`` is a contiguous 2-d CUDA float32 / float64 tensor on the model's device -- the
        periodic mass plane, or a window of it that the caller gathered -- and ``origin`` = (x0, y0), ``size`` the
        ``size`` x ``size`` window of it that is the tile, wrapped in the kernel; ``crop`` = (r0, c0, m) the footprint
        in the painted tile (``lightcone.small_plane_geometry``'s integers).  The window's minimum where
        ``subtract_minimum`` (bp_window_min), the spline zoom straight into slot 0's ``raw`` of
        ``model.paint_graph(1)`` (bp_window_zoom), the parameter block of one tile with ``paint_stream``'s seed word and
        ``tile_id`` -- with ``pixel_noise`` the lattice ``tile_id`` at origin (0, 0), as on the host path -- the replay,
        and the crop of label field ``field_index`` (None: the only one) of the slot's ``out`` (bp_tile_crop).  Returns
        the (m, m) float64 plane as NumPy, or ``out`` (a CUDA float64 (m, m) tensor) filled in place.

        ``draws`` = K (``lightcone.paint_small_plane_ensemble``; refusals, ``out``, ``return_planes`` and ``moments`` as in
        ``_paint_plane_device``): ``model.paint_graph(1, draws=K)`` with its draws, one crop per draw into (K, m, m) and
        ``bp_plane_moments`` across them.  Without ``draws`` nothing changes."""
        model = self.model
        model.train(False)
        tile, W = self._tile_shape()
        if tile != W:
            raise NotImplementedError("device planes need square tiles")
        if draws is not None:
            K = PG.check_draws(draws)
            params, scales, modes = self._ensemble_parameters(np.full(1, float(z)), pixel_noise)
            return _paint_small_plane_pipeline(self, model, tile, plane, origin, int(size), crop, params,
                                               np.array([tile_id], dtype=np.int64), seed, subtract_minimum, field_index,
                                               out, scales, modes, ensemble=(K, return_planes, moments))
        if pixel_noise:
            self._need_pixel_noise()
        params, scales, modes = self._device_paint_parameters(np.full(1, float(z)))
        ids = np.array([tile_id], dtype=np.int64)
        if pixel_noise:
            params = _with_noise(params, ids, None, 1, tile, tile, 0, 1)
        return _paint_small_plane_pipeline(self, model, tile, plane, origin, int(size), crop, params, ids, seed,
                                           subtract_minimum, field_index, out, scales, modes)


class CVAEPainter(Painter):
    def __init__(self, filename=None, training_data_set=None, test_data_set=None, architecture="test",
                 compute_device="cuda:0", sync=None, dtype="f32"):
        """The reference's arguments (painter.py:34-38) plus ``sync`` (data parallel, baryon_painter_amd.dist.Sync) and
        ``dtype``: "f32" = the reference's arithmetic, "bf16" = the bf16 throughput mode of ``models.cvae.CVAE``."""
        self.sync = sync
        self.dtype = dtype
        if filename is not None:
            self.load_state_from_file(filename, compute_device)
        else:
            self.architecture = architecture
            self.compute_device = compute_device
            self.model = _cvae.CVAE(architecture, torch.device(compute_device), sync=sync, dtype=dtype)
        self.training_data = training_data_set
        self.test_data = test_data_set

    def load_training_data(self, filename):
        self.data_path = os.path.dirname(filename)
        with open(filename, "rb") as f:
            self.training_data_file_info = pickle.load(f)

    def load_test_data(self, filename):
        self.test_data_path = os.path.dirname(filename)
        with open(filename, "rb") as f:
            self.test_data_file_info = pickle.load(f)

    # ------------------------------------------------------------------------------ training
    def _loader(self, batch_size):
        if self.sync is not None and self.sync.world_size > 1:
            return _ShardedLoader(self.training_data, batch_size, self.sync)
        if getattr(self, "device_assembler", None) is not None:
            return _DeviceLoader(self.device_assembler, len(self.training_data), batch_size)
        return torch.utils.data.DataLoader(self.training_data, batch_size=batch_size, shuffle=True)

    def use_device_assembly(self, k_values=None, mode="shift-log"):
        """Keep the training stacks in HBM and assemble batches on the device (utils.datasets.DeviceTileAssembler)
        instead of the host DataLoader; same shuffle order.  Without arguments the transform is read from the training
        set's chain: a range compression (any of the six modes, one per field), optionally followed by a split-scale
        transform (NotImplementedError for any other chain, before a stack is uploaded); ``subtract_minimum`` sets are served too.  ``k_values`` / ``mode`` given
        explicitly mean a single-scale shift-log (or, with ``mode=None``, untransformed) batch, as before."""
        self.device_assembler = datasets.DeviceTileAssembler(self.training_data, self.compute_device,
                                                             k_values=k_values, mode=mode)

    def train(self, n_epoch=5, n_pepoch=None, learning_rate=1e-4, batch_size=1,
              adaptive_learning_rate=None, adaptive_batch_size=None,
              validation_pepochs=[0, 1], validation_batch_size=4,
              validation_loss_frequency=100, validation_loss_batch_size=16,
              checkpoint_frequency=1000, statistics_report_frequency=50,
              loss_plot_frequency=1000, mavg_window_size=20,
              plot_sample_var=False, plot_power_spectra=["auto"], plot_histogram=["log"],
              show_plots=True, save_plots=False, output_path=None, verbose=True,
              pepoch_size=3136, var_anneal_fn=None, KL_anneal_fn=None, graph_step=False):
        """Train.  1 pseudo epoch = ``pepoch_size`` samples (3136 by default; the checked-in
        script uses 1568).  Returns ``(training_stats, validation_stats)``.

        ``graph_step=True`` (extension): forward + backward + Adam of full minibatches replay from one hipGraph
        (``CVAE.make_graphed_train_step``) - same arithmetic, ~2x the throughput at the reference's minibatch
        sizes of 4-24 tiles, where a step is bound by its ~450 kernel launches.  Single device only."""
        if self.training_data is None:
            raise RuntimeError("Trying to train but no training data specified.")
        if len(validation_pepochs) > 0 and self.test_data is None:
            raise RuntimeError("Trying to validate but no test data specified.")
        model = self.model
        model.train(True)
        if adaptive_batch_size is not None or batch_size <= 0:
            batch_size = adaptive_batch_size(0)
        dataloader = self._loader(batch_size)

        # torch.optim.Adam arithmetic, one fused launch over the flat parameter buffer
        from .optim import FlatAdam
        optimizer = FlatAdam(model, lr=learning_rate)
        scheduler = None
        if adaptive_learning_rate is not None:
            if callable(adaptive_learning_rate):
                scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, adaptive_learning_rate)
            elif isinstance(adaptive_learning_rate, dict):
                scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=adaptive_learning_rate["step_size"],
                                                            gamma=adaptive_learning_rate["gamma"])
            elif adaptive_learning_rate == "avoid_plateau":
                scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="max", factor=0.1,
                                                                       patience=10, threshold=0.0001,
                                                                       threshold_mode="rel", cooldown=0, min_lr=0,
                                                                       eps=1e-08)

        # statistics labels: "log_likelihood_0" -> "log_likelihood_pressure_0" (painter.py:114-121)
        nf = self.training_data.n_feature_per_field
        stats_labels = model.get_stats_labels()
        for j, f in enumerate(self.training_data.label_fields):
            for k in range(nf):
                stats_labels = [l.replace(f"{j * nf + k}", f"{f}_{k}") for l in stats_labels]
        stats_labels += ["lr", "batch_size"]

        ckpt_template = train_file = val_file = idx_file = None
        if output_path is not None:
            os.makedirs(output_path, exist_ok=True)
            ckpt_template = os.path.join(output_path, "checkpoint_sample{sample:0>10}_batch{batch}_epoch{epoch}{suffix}")
            train_file = os.path.join(output_path, "training_stats.txt")
            val_file = os.path.join(output_path, "validation_stats.txt")
            idx_file = os.path.join(output_path, "training_sample_indicies.txt")
        elif save_plots:
            raise ValueError("save_plots=True requires output_path to be set.")
        rank0 = self.sync is None or self.sync.rank == 0
        if not rank0:
            ckpt_template = train_file = val_file = idx_file = None

        training_stats = TrainingStats(stats_labels, mavg_window_size, stats_filename=train_file)
        validation_stats = TrainingStats(stats_labels, mavg_window_size, stats_filename=val_file,
                                         dump_to_file_frequency=1)
        if n_pepoch is None:
            n_pepoch = n_epoch * len(self.training_data) // pepoch_size

        sample_indices = []
        n_samples = n_batches = 0
        last_pepoch_at = last_val = last_report = last_ckpt = 0
        i_epoch = i_pepoch = i_batch = 0
        world = 1 if self.sync is None else self.sync.world_size
        ELBO = None
        graphed_steps = {}

        while i_epoch < n_epoch:
            i_epoch = n_samples // len(self.training_data)
            if verbose:
                model.check_gpu()
            if i_pepoch >= n_pepoch:
                break
            for i_batch, batch_data in enumerate(dataloader):
                if n_samples - pepoch_size >= last_pepoch_at or n_samples == 0:
                    if n_samples != 0:
                        i_pepoch += 1
                        last_pepoch_at = n_samples
                        if i_pepoch >= n_pepoch:
                            break
                        if scheduler is not None:
                            if adaptive_learning_rate == "avoid_plateau":
                                scheduler.step(float(ELBO.item()))
                            else:
                                scheduler.step()
                    if callable(var_anneal_fn):
                        model.alpha_var = var_anneal_fn(i_pepoch)
                    if callable(KL_anneal_fn):
                        model.beta_KL = KL_anneal_fn(i_pepoch)
                    if i_pepoch in validation_pepochs:
                        self.validate(validation_batch_size=validation_batch_size, plot_sample_var=plot_sample_var)
                    if adaptive_batch_size is not None:
                        new_bs = adaptive_batch_size(i_pepoch)
                        if new_bs != batch_size:
                            batch_size = new_bs
                            dataloader = self._loader(batch_size)
                            break

                x = torch.cat(batch_data[0][1:], dim=1).to(model.device)
                y = batch_data[0][0].to(model.device)
                aux = batch_data[2].to(device=model.device, dtype=y.dtype) if len(batch_data) > 2 else None

                if graph_step and self.sync is None:
                    n_b = int(y.shape[0])
                    if n_b not in graphed_steps and n_b == batch_size:
                        graphed_steps[n_b] = model.make_graphed_train_step(optimizer, n_b)
                    stepper = graphed_steps.get(n_b)
                else:
                    stepper = None
                if stepper is not None:
                    if callable(var_anneal_fn) or callable(KL_anneal_fn):
                        raise NotImplementedError("graph_step with annealed loss weights (they are captured constants)")
                    ELBO = stepper(x, y, aux)
                else:
                    ELBO = model(x, y, aux)
                    optimizer.zero_grad()
                    (-ELBO).backward()
                    optimizer.step()

                n_samples += x.size(0) * world
                n_batches += 1
                with torch.no_grad():
                    sample_indices += list(np.asarray(batch_data[1]))
                    lr = [g["lr"] for g in optimizer.param_groups]
                    training_stats.push_loss(n_samples, *model.get_stats(), lr[0], batch_size)
                    if n_samples - validation_loss_frequency >= last_val:
                        last_val = n_samples
                        stats = self.validate(validation_batch_size=validation_loss_batch_size, compute_loss=True)
                        validation_stats.push_loss(n_samples, *stats, lr[0], batch_size)
                    if n_samples - checkpoint_frequency >= last_ckpt and ckpt_template is not None:
                        last_ckpt = n_samples
                        base = ckpt_template.format(epoch=i_epoch, batch=i_batch, sample=n_samples, suffix="")
                        self.save_state_to_file((base + "_state", base + "_meta"))
                    if n_samples - statistics_report_frequency >= last_report and statistics_report_frequency > 0:
                        last_report = n_samples
                        if rank0:
                            print("Epoch: [{}/{}], P-Epoch: [{}/{}], Batch: [{}/{}], Loss: {:.3e}".format(
                                i_epoch, n_epoch, i_pepoch, n_pepoch, i_batch,
                                len(self.training_data) // (batch_size * world),
                                training_stats.loss_terms["ELBO"]["mavg"][-1]))
                            print("Processed batches: {}, processed samples: {}, batch size: {}, learning rate: {}"
                                  .format(n_batches, n_samples, batch_size, " ".join("{:.1e}".format(v) for v in lr)))
                            print(training_stats.get_pretty_str(n_col=1))
                        if idx_file is not None:
                            with open(idx_file, "wb") as f:
                                pickle.dump(sample_indices, f)

        self.validate(validation_batch_size=validation_batch_size, plot_sample_var=plot_sample_var)
        if ckpt_template is not None:
            base = ckpt_template.format(epoch=i_epoch, batch=i_batch, sample=n_samples, suffix="_final")
            self.save_state_to_file((base + "_state", base + "_meta"))
            self.save_state_to_file((os.path.join(output_path, "model_state"), os.path.join(output_path, "model_meta")))
        training_stats.flush_to_file()
        validation_stats.flush_to_file()
        return training_stats, validation_stats

    def validate(self, validation_batch_size=8, compute_loss=False, validation_redshift=None,
                 plot_samples=1, plot_sample_var=False, plot_power_spectra=["auto"], plot_histogram=["log"],
                 histogram_n_sample=1, show_plots=True, save_plots=False, filename_template="{plot_type}.png"):
        """A random test batch through the model (painter.py:295-367).  With ``compute_loss`` the
        loss terms (``model.get_stats()``) are returned; otherwise the reference draws diagnostic
        plots from a prior sample -- here the sample is drawn (same device work, same random
        stream) and returned as ``(x, y, x_pred[, x_pred_var])`` NumPy arrays instead."""
        model = self.model
        with torch.no_grad():
            fields, indicies, z = self.test_data.get_batch(size=validation_batch_size, z=validation_redshift)
            x = torch.tensor(np.concatenate(fields[1:], axis=1), device=model.device)
            y = torch.tensor(fields[0], device=model.device)
            aux = torch.tensor(z, device=model.device, dtype=y.dtype)
            if compute_loss:
                model(x, y, aux)
                return model.get_stats()
            if plot_sample_var and model.predict_var:
                x_pred, x_var = model.sample_P(y, return_var=True, aux_label=aux)
                return x.cpu().numpy(), y.cpu().numpy(), x_pred.cpu().numpy(), x_var.cpu().numpy()
            x_pred = model.sample_P(y, aux_label=aux)
            return x.cpu().numpy(), y.cpu().numpy(), x_pred.cpu().numpy()

    # ------------------------------------------------------------------------------ inference
    def _inverse_fields(self, head, z):
        """One tile's head (F * nf, H, W) of a painter with F > 1 label fields -> (F, H, W) physical tiles: field j owns
        channels [j * nf, (j + 1) * nf) and is inverted as ``label_fields[j]`` (the reference's slicing,
        validation_plotting.py:109-110)."""
        F = len(self.label_fields)
        if head.shape[0] % F:
            raise ValueError(f"a head of {head.shape[0]} channels does not split into {F} label fields")
        nf = head.shape[0] // F
        return np.stack([self.inverse_transform(head[j * nf:(j + 1) * nf][None] if nf == 1 else head[j * nf:(j + 1) * nf],
                                                field=f, z=z) for j, f in enumerate(self.label_fields)])

    def _need_pixel_noise(self):
        self.model._need_var_head("pixel_noise=True")

    @staticmethod
    def _fresh_seed(seed):
        """``seed``, or a fresh Philox key from torch's global generator (as ``lightcone.paint_plane`` draws one)."""
        return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed

    def paint(self, input, z=0.0, transform=True, inverse_transform=True, pixel_noise=False, seed=None, noise_id=0,
              noise_origin=(0, 0)):
        """Paint one tile (painter.py:371-392): dark-matter tile (H,W) at redshift z -> pressure.  A painter with F > 1
        label fields returns (F, H, W), field j from head channels [j * nf, (j + 1) * nf) (where the reference raises
        NotImplementedError, painter.py:388-389); ``inverse_transform=False`` gives the (1, F * nf, H, W) head.

        ``pixel_noise=True`` (a model with a variance head; ValueError otherwise): the tile is a draw from the
        likelihood, x_mu + sqrt(x_var) e in network units, not its mean -- ``paint_stream``'s noise: Philox under the key
        ``seed`` (None: a fresh key from torch's global generator) on the lattice ``noise_id``, window origin
        ``noise_origin`` = (row, col)."""
        self.model.train(False)
        noise = None
        if pixel_noise:
            self._need_pixel_noise()
            noise = {"seed": self._fresh_seed(seed), "ids": np.array([noise_id], dtype=np.int64),
                     "origins": np.asarray(noise_origin).reshape(1, 2)}
        with torch.no_grad():
            y = self.transform(input, field=self.input_field, z=z) if transform and self.transform is not None \
                else input
            y = np.asarray(y)
            y = y.reshape(1, *y.shape)
            if y.shape != (1, *self.model.dim_y):
                raise ValueError(f"Shape mismatch between input and model: {input.shape} vs {self.model.dim_y}")
            yt = torch.tensor(y, device=self.compute_device, dtype=torch.float32)
            aux = torch.tensor(z, device=self.compute_device, dtype=yt.dtype)
            prediction = self.model.sample_P(yt, aux_label=aux, pixel_noise=noise).cpu().numpy()
        if inverse_transform and self.inverse_transform is not None:
            if len(self.label_fields) > 1:
                return self._inverse_fields(prediction[0], z)
            if prediction.shape[1] != 1:       # a multi-scale head: the inverse takes one tile's (cx, H, W) channels
                return self.inverse_transform(prediction[0], field=self.label_fields[0], z=z)
            return self.inverse_transform(prediction, field=self.label_fields[0], z=z)
        return prediction

    def paint_batch(self, inputs, z, transform=True, inverse_transform=True, batch_size=64, use_graph=True,
                    pixel_noise=False, seed=None, noise_ids=None, noise_origins=None):
        """Throughput form of ``paint``: many tiles (N,H,W) with redshifts (N,) in batches through the
        same eval-mode forward (BASELINE.json configs[4]); per-tile results equal ``paint``'s up to
        the prior noise draw.  (N, H, W), or (N, F, H, W) for a painter with F > 1 label fields, each field through
        its own inverse (``_inverse_fields``).

        ``pixel_noise=True``: draws from the likelihood as in ``paint``, tile i on the lattice ``noise_ids[i]``
        [default: i] at ``noise_origins[i]`` [default: (0, 0)] under the key ``seed`` (None: a fresh one); these batches
        go through ``sample_P`` (the graphed form has no draw)."""
        self.model.train(False)
        inputs = np.asarray(inputs)
        zs = np.broadcast_to(np.asarray(z, dtype=np.float64), (inputs.shape[0],))
        if pixel_noise:
            self._need_pixel_noise()
            N = inputs.shape[0]
            n_ids, n_org = PG.noise_lattice(np.arange(N, dtype=np.int64) if noise_ids is None else noise_ids,
                                            noise_origins, N, *self.model.dim_x[1:])
            seed = self._fresh_seed(seed)
        out = []
        with torch.no_grad():
            for s in range(0, inputs.shape[0], batch_size):
                chunk = inputs[s:s + batch_size]
                zc = zs[s:s + batch_size]
                if transform and self.transform is not None:
                    y = np.stack([np.asarray(self.transform(t, field=self.input_field, z=float(zz)))
                                  for t, zz in zip(chunk, zc)])
                else:
                    y = chunk.reshape(chunk.shape[0], 1, *chunk.shape[-2:])
                y = y.reshape(y.shape[0], *self.model.dim_y)
                yt = torch.tensor(y, device=self.compute_device, dtype=torch.float32)
                aux = torch.tensor(zc, device=self.compute_device, dtype=torch.float32)
                graphed = use_graph and self.model._eps_override is None and yt.shape[0] == batch_size
                if pixel_noise:
                    e = s + yt.shape[0]
                    pred = self.model.sample_P(yt, aux_label=aux, pixel_noise={
                        "seed": seed, "ids": n_ids[s:e], "origins": None if n_org is None else n_org[s:e]}).cpu().numpy()
                else:
                    sample = self.model.sample_P_graphed if graphed else self.model.sample_P
                    pred = sample(yt, aux_label=aux).cpu().numpy()
                if inverse_transform and self.inverse_transform is not None and len(self.label_fields) > 1:
                    pred = np.stack([self._inverse_fields(p, float(zz)) for p, zz in zip(pred, zc)])
                elif inverse_transform and self.inverse_transform is not None:
                    pred = np.stack([self.inverse_transform(p[None] if p.shape[0] == 1 else p,
                                                            field=self.label_fields[0], z=float(zz))
                                     for p, zz in zip(pred, zc)])
                out.append(pred)
        return np.concatenate(out, axis=0)

    # ---- throughput pipeline (BASELINE.json configs[4]) ---------------------------------------------------------
    def _transform_parameters(self, zs, records=False):
        """(params, scales, modes) for the device-side transforms, read out of the compiled host transforms: per tile
        the parameter rows ``xf_in`` / ``xf_out`` of the reference's range compression (data_transforms.py:72-108) for
        ``CVAE.paint_graph``'s block, the description of a multi-scale painter's split-scale transform (``paint_graph``'s
        ``scales``) or None, and ``modes``: None where both fields are "shift-log" (rows {sigma, k} / {k, sigma}, the
        pipeline as it always was), else the (input, label) mode numbers (rows: the four-double records of
        csrc/range_compress.hpp).  With F > 1 label fields ``xf_out`` is (n, F, 4), the records of each field, and
        ``modes`` is (input mode, (mode of field 0, ...)): the four-double form on both sides whatever the modes are;
        every field's inverse chain must have a device form, and all of them share the split-scale parameters.
        ``records=True`` (an ensemble, ``paint_ensemble``): the four-double records and both mode numbers also where both
        fields are "shift-log".  Anything else has no device form.  The chains with one:
          single scale   any order of ONE range compression and the shape-only steps;
          multi scale    forward  [range compression, as_float32 (optional), split-scale, shape-only steps ...]
                         inverse  [inverse split-scale, inverse range compression, shape-only steps ...]
                         with the same split-scale parameters on both sides -- exactly these orders: the kernels
                         filter the transformed tile and sum in front of the inverse transform.
        (The chains are read by ``data_transforms.device_shift_log`` / ``device_split_scale``, which the training-side
        ``datasets.DeviceTileAssembler`` shares.)"""
        from .utils import data_transforms as T

        def func_of(compiled):
            if compiled is None:
                raise NotImplementedError("paint_stream needs the painter's transforms (transform=None has no device form)")
            return getattr(compiled, "func", None)

        def find(compiled, direction, field):
            return T.device_shift_log(func_of(compiled), direction, field), compiled.stats[field]

        def find_scales(compiled, direction, field):
            """The strict multi-scale orders; returns (range compression, split-scale step)."""
            rc, split = T.device_split_scale(func_of(compiled), direction, field)
            return (rc, compiled.stats[field]), split

        def has_split(compiled):
            return compiled is not None and T.has_split_scale(getattr(compiled, "func", None))
        if len(self.label_fields) < 1:
            raise NotImplementedError("a painter without a label field has nothing to paint")
        scales = None
        outs = []                                      # per label field: (range compression, the field's statistics)
        if has_split(self.transform) or has_split(self.inverse_transform):
            (rc_in, st_in), fs = find_scales(self.transform, 0, self.input_field)
            for f in self.label_fields:
                out_f, bs = find_scales(self.inverse_transform, 1, f)
                outs.append(out_f)
                if (fs.n_scale, fs.include_original) != (bs.n_scale, bs.include_original):
                    raise NotImplementedError("the split-scale transform and its inverse differ in n_scale / "
                                              "include_original")
            scales = {"n_scale": fs.n_scale, "step_size": fs.step_size, "include_original": fs.include_original,
                      "truncate": fs.truncate}
        else:
            rc_in, st_in = find(self.transform, 0, self.input_field)
            outs = [find(self.inverse_transform, 1, f) for f in self.label_fields]
        if len(outs) > 1:
            # several label fields: records on both sides, one (n, 4) table per field side by side, and every field's mode
            xf_out = np.stack([rc.records(st, zs) for rc, st in outs], axis=1)
            return ({"xf_in": rc_in.records(st_in, zs), "xf_out": xf_out, "aux": np.asarray(zs, dtype=np.float64)}, scales,
                    (rc_in.mode, tuple(rc.mode for rc, _ in outs)))
        rc_out, st_out = outs[0]
        xf_in, xf_out = rc_in.records(st_in, zs), rc_out.records(st_out, zs)      # (vectorised: no Python call per tile)
        modes = (rc_in.mode, rc_out.mode)
        if rc_in.name == rc_out.name == "shift-log" and not records:
            modes, xf_in, xf_out = None, xf_in[:, :2], xf_out[:, 1::-1]
        return {"xf_in": xf_in, "xf_out": xf_out, "aux": np.asarray(zs, dtype=np.float64)}, scales, modes

    def _tile_shape(self):
        return tuple(self.model.dim_y[1:])

    def _shape_mismatch(self, shape):
        return f"Shape mismatch between input and model: {shape} vs {self.model.dim_y}"

    def _device_paint_parameters(self, zs, ensemble=False):
        """``_transform_parameters(zs)`` where this painter has a device form -- one of the six range compressions on
        either side (one per label field), with or without a prior network or a p_y_in network, a split-scale transform
        in the orders ``_transform_parameters`` names, and a model the captured pipeline takes
        (``paint_graph.paint_levels``: channels, L = 1, no split-scale with a p_y_in network) -- and NotImplementedError
        where it has none.  No side effects.  ``ensemble`` (``paint_ensemble``: the number of draws is its argument, not
        the model's): any L, and ``_transform_parameters(zs, records=True)``."""
        model = self.model
        params, scales, modes = self._transform_parameters(zs, records=ensemble)
        PG.paint_levels(model.dim_y[0], model.dim_x[0], getattr(model, "has_p_y_in", False), getattr(model, "L", 1),
                        scales, len(self.label_fields), ensemble, mismatch=NotImplementedError)
        return params, scales, modes

    def paint_ensemble(self, inputs, z, draws, batch_size=64, tile_ids=None, seed=0, rank=0, world_size=1,
                       return_draws=False, pixel_noise=False, noise_ids=None):
        """The conditional mean and scatter of the painted field at fixed dark matter: ``draws`` = K (1 ... 64) latent
        draws per raw tile of ``inputs`` (N, H, W), reduced on the device -> (mean, var), float32 (N, H, W) each, or
        (N, F, H, W) for F > 1 label fields; ``var`` is the population variance over the K draws (``np.var``, ddof = 0),
        both accumulated in float64 over the float32 physical tiles a single painting stores
        (``bp_paint_store_moments``).  ``return_draws=True`` adds the draws themselves, (N, K, [F,] H, W).

        It is ``paint_stream``'s pipeline -- pinned double buffers, two slots, one parameter-block copy per batch, the
        seed read from the device -- over ``model.paint_graph(batch_size // K, draws=K)``: ``batch_size`` counts
        generator samples as everywhere else, so a batch carries ``batch_size // K`` tiles (K must divide it), and the
        load, the pyramid, p_y_in and the prior network run once per TILE.  Draw k of tile id t uses the Philox counter
        (g, k, t): draw 0 is the tile ``paint_stream`` paints for the same seed and id, and no draw depends on batches
        or ranks.  The model may have any ``L``.  ``rank`` / ``world_size`` shard tiles as in ``paint_stream`` (the
        result is then (arrays, (lo, hi))).  ``pixel_noise=True`` (a variance head; ValueError otherwise): every draw is
        also a draw from the likelihood, draw k of a tile on the lattice ``noise_ids[i]`` [default: ``tile_ids[i]``] +
        (k << 40) at the origin (0, 0); the ids must lie in [0, 2^40) (ValueError before any capture).

        These are the moments of TILES.  The moments of a feathered blend of overlapping tiles are not the blend of the
        tiles' moments (the blend runs in physical units behind a non-linear inverse), so planes and light cones do
        not blend ``mean`` and ``var``: ``lightcone.paint_plane_ensemble``, ``paint_small_plane_ensemble`` and
        ``paint_light_cone_ensemble`` blend, or project, every draw on its own and take the moments across the K
        planes, or y maps."""
        K = PG.check_draws(draws)
        B = int(batch_size)
        if B < K or B % K:
            raise ValueError(f"batch_size counts generator samples: {K} draws per tile must divide it, got {batch_size}")
        if pixel_noise:                                   # (checked before the model is touched)
            self._need_pixel_noise()
            N = len(inputs)
            lattice = np.asarray(noise_ids) if noise_ids is not None else \
                np.arange(N, dtype=np.int64) if tile_ids is None else np.asarray(tile_ids, dtype=np.int64)
            if lattice.shape != (N,):
                raise ValueError(f"noise ids must be {N} integers, got shape {lattice.shape}")
            PG.ensemble_noise_ids(lattice, 1)             # (the range check, before any capture)
        model, (H, W), N, zs, ids, lo, hi = self._stream_prologue(inputs, z, tile_ids, rank, world_size)
        params, scales, modes = self._device_paint_parameters(zs[lo:hi], ensemble=True)
        if pixel_noise:
            params = dict(params, noise_ids=lattice[lo:hi].astype(np.int64))
        result = _paint_stream_pipeline(self, model, inputs, (H, W), lo, hi, B // K, params, ids[lo:hi], seed, None, scales,
                                        modes, ensemble={"draws": K, "return_draws": bool(return_draws)})
        return (result, (lo, hi)) if world_size > 1 else result

    def can_paint_stream(self, z=0.0):
        """Whether ``paint_stream`` has a device form for this painter (``_device_paint_parameters``) -- WITHOUT side
        effects: nothing is captured, no random number is drawn.  ``lightcone.paint_plane`` asks this before it draws a
        plane's seed, so that a NotImplementedError raised later, from inside a capture, is an error and not a silent
        fall-back."""
        try:
            self._device_paint_parameters(np.atleast_1d(np.asarray(z, dtype=np.float64))[:1])
        except NotImplementedError:
            return False
        return True

    # ---- scoring on held-out tiles -----------------------------------------------------------------
    def _score_parameters(self, zs):
        """(input mode, label modes, input records (n, 4), label records (F, n, 4)) of the FORWARD transforms of the
        input field and of every label field, for tiles at redshifts ``zs`` -- what ``score`` / ``reconstruct`` load
        raw tiles with on the device.  NotImplementedError, without side effects, for a painter that has no such form: a
        split-scale (multi-scale) painter, a chain ``data_transforms.device_shift_log`` does not read, or a model whose
        channels are not one per field."""
        from .utils import data_transforms as T
        tr = self.transform
        func = None if tr is None else getattr(tr, "func", None)
        if tr is None:
            raise NotImplementedError("score needs the painter's transforms (transform=None has no device form)")
        if T.has_split_scale(func) or T.has_split_scale(getattr(self.inverse_transform, "func", None)):
            raise NotImplementedError("score has no device form for a split-scale painter: transform on the host and "
                                      "call model.score")
        F = len(self.label_fields)
        if F < 1 or self.model.dim_y[0] != 1 or self.model.dim_x[0] != F:
            raise NotImplementedError(f"score needs one channel per field, the model has dim_y {self.model.dim_y} and "
                                      f"dim_x {self.model.dim_x} for {F} label fields")
        rc_in = T.device_shift_log(func, 0, self.input_field)
        rcs = [T.device_shift_log(func, 0, f) for f in self.label_fields]
        rec_x = np.stack([rc.records(tr.stats[f], zs) for rc, f in zip(rcs, self.label_fields)])
        return rc_in.mode, [rc.mode for rc in rcs], rc_in.records(tr.stats[self.input_field], zs), rec_x

    def can_score(self, z=0.0):
        """Whether ``score`` / ``reconstruct`` have a device form for this painter, WITHOUT side effects (as
        ``can_paint_stream``): nothing is built, no random number is drawn."""
        try:
            self._score_parameters(np.atleast_1d(np.asarray(z, dtype=np.float64))[:1])
        except NotImplementedError:
            return False
        return True

    def _score_batches(self, inputs, truths, z, tile_ids, seed, per_batch, K, lo, hi, run):
        """Batches of ``per_batch`` tiles of [lo, hi) through ``run(plan, eps or None, a, b)``: per batch ONE pinned
        upload (raw tiles, raw truths, records, redshifts, tile ids and the seed in one block), the forward transforms on
        the device (``bp_paint_load_mode`` with each field's own record, the truths into their channel slices of the
        plan's ``x_in`` slot), and -- where ``K`` is not None -- the normals of counter (g, k, tile id) under ``seed``."""
        import ctypes as C
        from . import _lib as L
        from .models.graph import _stream
        model = self.model
        dev, lib = model.device, model._lib
        H, W = self._tile_shape()
        F = len(self.label_fields)
        zs = np.broadcast_to(np.asarray(z, dtype=np.float64), (len(inputs),))
        ids = np.arange(len(inputs), dtype=np.int64) if tile_ids is None else np.asarray(tile_ids, dtype=np.int64)
        mode_in, modes_x, _, _ = self._score_parameters(zs[:1])
        per_tile = int(np.prod(model.dim_z))
        caux = model.n_aux if model.use_aux_label else 0
        blocks = self.__dict__.setdefault("_score_buffers", {})     # (page-locking costs tens of milliseconds: kept)
        with torch.no_grad():
            for a in range(lo, hi, per_batch):
                b = min(a + per_batch, hi)
                n = b - a
                _, _, rec_in, rec_x = self._score_parameters(zs[a:b])
                parts = [("raw", np.float32, (n, 1, H, W)), ("truth", np.float32, (F, n, H, W)),
                         ("rec_in", np.float64, (n, 4)), ("rec_x", np.float64, (F, n, 4)), ("ids", np.int64, (n,)),
                         ("seed", np.int64, (1,)), ("aux", np.float32, (n, 1))]
                if (n, F, H, W) not in blocks:
                    off, layout = 0, {}
                    for name, dt, shape in parts:
                        layout[name] = (off, dt, shape)
                        off += -(-int(np.prod(shape)) * np.dtype(dt).itemsize // 16) * 16
                    host = torch.zeros(off, dtype=torch.uint8).pin_memory()
                    blocks[(n, F, H, W)] = (layout, host, torch.zeros(off, dtype=torch.uint8, device=dev),
                                            torch.zeros((n, 1, H, W), device=dev))
                layout, host, block, y_t = blocks[(n, F, H, W)]
                hv = host.numpy()

                def field(buf, name, layout=layout):
                    """The typed view of one part of the block: of the host mirror (NumPy) or of the device copy."""
                    off, dt, shape = layout[name]
                    size = int(np.prod(shape)) * np.dtype(dt).itemsize
                    if isinstance(buf, torch.Tensor):
                        return buf[off:off + size].view(getattr(torch, np.dtype(dt).name)).view(shape)
                    return buf[off:off + size].view(dt).reshape(shape)
                field(hv, "raw")[:, 0] = np.asarray(inputs[a:b], dtype=np.float32)
                tr_ab = np.asarray(truths[a:b], dtype=np.float32).reshape(n, F, H, W)
                field(hv, "truth")[:] = tr_ab.transpose(1, 0, 2, 3)
                field(hv, "rec_in")[:] = rec_in
                field(hv, "rec_x")[:] = rec_x
                field(hv, "ids")[:] = ids[a:b]
                field(hv, "seed")[0] = PG.seed_word(seed)
                field(hv, "aux")[:, 0] = zs[a:b]
                block.copy_(host, non_blocking=True)
                plan = model._score_plan(n, 1 if K is None else K, "score")
                st = _stream()
                L.check(lib.bp_paint_load_mode(mode_in, L.ptr(field(block, "raw")), 1, L.ptr(field(block, "rec_in")), None,
                                               0, C.byref(L.view(y_t, n, H, W, 1)), st), "load y")
                plan.load_inputs(y_t, field(block, "aux") if caux else None, None, False)
                truth_d, rec_d = field(block, "truth"), field(block, "rec_x")
                for j in range(F):
                    v = L.view(plan.x_in.buf, n, H, W, 1, plan.x_in.cstride, plan.x_in.coff + j)
                    L.check(lib.bp_paint_load_mode(modes_x[j], L.ptr(truth_d[j]), 1, L.ptr(rec_d[j]), None, 0, C.byref(v),
                                                   st), "load x")
                if plan.x_nchw.data_ptr() != plan.x_in.buf.data_ptr():
                    L.check(lib.bp_view_to_nchw(C.byref(plan.x_in.view), None, 0, L.ptr(plan.x_nchw), st), "x layout")
                eps = None
                if K is not None:
                    eps = torch.empty((K, n, *model.dim_z), device=dev)
                    L.check(lib.bp_philox_normal_dev(L.ptr(field(block, "seed")), L.ptr(field(block, "ids")), n, K,
                                                     per_tile, L.ptr(eps), st), "philox")
                run(plan, eps, a, b)
                torch.cuda.current_stream(dev).synchronize()      # (the pinned block is rewritten by the next batch)

    def _score_prologue(self, inputs, truths, z, rank, world_size):
        """Shapes checked (ValueError), the device form checked (NotImplementedError), the model in eval mode; returns
        this rank's share [lo, hi) of the N tiles.  Nothing is built, no random number is drawn."""
        H, W = self._tile_shape()
        F = len(self.label_fields)
        N = len(inputs)
        self._score_parameters(np.atleast_1d(np.asarray(z, dtype=np.float64))[:1])
        if tuple(np.shape(inputs)[1:]) != (H, W):
            raise ValueError(self._shape_mismatch(tuple(np.shape(inputs))))
        if tuple(np.shape(truths)) not in ([(N, F, H, W)] + ([(N, H, W)] if F == 1 else [])):
            raise ValueError(f"truths have shape {tuple(np.shape(truths))}, expected {(N, F, H, W)}")
        self.model.train(False)
        per = (N + world_size - 1) // world_size
        return N, min(rank * per, N), min((rank + 1) * per, N)

    def score(self, inputs, truths, z, draws=16, batch_size=64, tile_ids=None, seed=0, rank=0, world_size=1):
        """Score this painter on held-out tiles: raw dark-matter tiles ``inputs`` (N, H, W) and the raw truth of every
        label field, ``truths`` (N, H, W) or (N, F, H, W), at redshifts ``z`` -> a dict of float64 arrays (N,) with the
        keys ``bound``, ``elbo``, ``log_likelihood``, ``kl`` and ``ess`` (``CVAE.score``'s columns: the per-tile evidence
        lower bound in eval mode, tightened by ``draws`` = K importance-weighted draws from the recognition network).
        Values are nats in NETWORK units -- they compare painters that share a transform and carry no Jacobian to
        physical units.

        ``batch_size`` counts generator samples, as in ``paint_ensemble``: a batch carries ``batch_size // K`` tiles and K
        must divide it (ValueError).  Draw k of tile id t (``tile_ids``, default 0 ... N - 1) uses the Philox counter
        (g, k, t) under ``seed``, so nothing depends on batches or ranks; ``rank`` / ``world_size`` shard the tiles as in
        ``paint_stream`` (the result is then (dict, (lo, hi))).  The forward transforms run on the device, each field
        with its own record (any of the six range compressions); a split-scale painter or a chain without a device form
        raises NotImplementedError before any device work (``can_score``): transform on the host and call
        ``model.score``."""
        K = PG.check_draws(draws)
        B = int(batch_size)
        if B < K or B % K:
            raise ValueError(f"batch_size counts generator samples: {K} draws per tile must divide it, got {batch_size}")
        N, lo, hi = self._score_prologue(inputs, truths, z, rank, world_size)
        out = np.zeros((hi - lo, 5), np.float64)

        def run(plan, eps, a, b):
            out[a - lo:b - lo] = self.model._score_loaded(plan, eps).cpu().numpy()
        self._score_batches(inputs, truths, z, tile_ids, seed, B // K, K, lo, hi, run)
        result = {k: np.ascontiguousarray(out[:, j]) for j, k in enumerate(SCORE_KEYS)}
        return (result, (lo, hi)) if world_size > 1 else result

    def reconstruct(self, inputs, truths, z, batch_size=64, sample=False, seed=0, tile_ids=None):
        """Encode the truth, decode it, in physical units: what the generator can express of ``truths`` -- tiles shaped as
        ``paint_batch`` returns them.  Inputs and the device loads are ``score``'s; the head (``model.reconstruct``) goes
        through the inverse transform exactly as ``paint_batch`` applies it.  ``sample=False``: the posterior mean,
        z = z_mu; ``sample=True``: one draw, draw 0 of the Philox counter (g, 0, tile id) under ``seed``."""
        N, lo, hi = self._score_prologue(inputs, truths, z, 0, 1)
        zs = np.broadcast_to(np.asarray(z, dtype=np.float64), (N,))
        out = []

        def run(plan, eps, a, b):
            if eps is None:
                eps = torch.zeros((1, plan.n, *self.model.dim_z), device=self.model.device)
            pred = self.model._reconstruct_loaded(plan, eps).cpu().numpy()
            if self.inverse_transform is not None and len(self.label_fields) > 1:
                pred = np.stack([self._inverse_fields(p, float(zz)) for p, zz in zip(pred, zs[a:b])])
            elif self.inverse_transform is not None:
                pred = np.stack([self.inverse_transform(p[None] if p.shape[0] == 1 else p, field=self.label_fields[0],
                                                        z=float(zz)) for p, zz in zip(pred, zs[a:b])])
            out.append(pred)
        self._score_batches(inputs, truths, z, tile_ids, seed, int(batch_size), 1 if sample else None, lo, hi, run)
        return np.concatenate(out, axis=0)

    def release_paint_buffers(self):
        """``Painter.release_paint_buffers``, a multi-scale pipeline's pyramid scratch, and the pinned and device blocks
        ``score`` / ``reconstruct`` keep per batch shape."""
        super().release_paint_buffers()
        self.__dict__.pop("_score_buffers", None)
        if hasattr(self.model, "release_scale_buffers"):
            self.model.release_scale_buffers()

    # ------------------------------------------------------------------------------ checkpoints
    def save_state_to_file(self, filename, mode="model_state_dict+metadata"):
        """(state_path, meta_path): ``torch.save(state_dict)`` + pickled metadata with the
        compiled transforms (painter.py:395-418).  The state dict has the reference's keys."""
        if not isinstance(filename, (tuple, list)):
            raise ValueError("filename needs to be a tuple of (state_filename, meta_filename).")
        td = self.training_data
        d = {"L": td.L, "n_grid": td.n_grid, "tile_L": td.tile_L, "n_tile": td.n_tile, "tile_size": td.tile_size,
             "input_field": td.input_field, "label_fields": td.label_fields, "scale_to_SLICS": td.scale_to_SLICS,
             "transform": datasets.compile_transform(transform=td.transform_func, stats=td.stats),
             "inverse_transform": datasets.compile_transform(transform=td.inverse_transform_func, stats=td.stats),
             "model_architecture": self.architecture}
        with open(filename[1], "wb") as f:
            _pickler.dump(d, f)
        torch.save({k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}, filename[0])

    def load_state_from_file(self, filename, compute_device="cuda:0"):
        if not isinstance(filename, (tuple, list)):
            raise ValueError("filename needs to be a tuple of (state_filename, meta_filename).")
        self.compute_device = compute_device
        state_dict = torch.load(filename[0], map_location=torch.device(self.compute_device))
        with open(filename[1], "rb") as f:
            d = _pickler.load(f)
        self.model = _cvae.CVAE(d["model_architecture"], torch.device(self.compute_device),
                                sync=getattr(self, "sync", None), dtype=getattr(self, "dtype", "f32"))
        self.model.load_state_dict(state_dict)
        self.architecture = d["model_architecture"]
        for k in ("L", "n_grid", "tile_L", "n_tile", "tile_size", "input_field", "label_fields", "scale_to_SLICS"):
            setattr(self, k, d[k])
        self.transform = d.get("transform")
        self.inverse_transform = d.get("inverse_transform")

# ---------------------------------------------------------------------------------------------------------------------
# The device paint pipelines, shared by the painters whose model has a ``paint_graph(B)`` (models.cvae.CVAE,
# models.cgan.CGAN): the models differ in what their captured graph does and in the columns of the transform
# parameters, not in how batches are fed to it.  ``params``: per tile of this call, ``xf_in`` / ``xf_out`` (n, k) float64
# rows of the graph's ``block_layout`` and ``aux`` (n,) the value of its conditioning plane.  ``params`` that also hold
# ``noise_ids`` (n,) int64 and ``noise_org`` (n, 2) int32 (``_with_noise``) select the graph that paints with pixel noise.

def _fill_block(hv, params, ids, a, b, B):
    """Tiles [a, b) of ``params`` / ``ids`` into the views of one block of ``B`` rows."""
    m = b - a
    hv["xf_in"][:m] = params["xf_in"][a:b]
    hv["xf_out"][:m] = params["xf_out"][a:b].reshape(m, -1)       # (several label fields: (m, F, 4) -> (m, 4 F))
    hv["aux"][:m, 0] = params["aux"][a:b]
    hv["tile_ids"][:m] = ids[a:b]
    keys = ("xf_in", "xf_out", "aux", "tile_ids")
    if "noise_ids" in params and hv["noise_ids"].ndim == 3:
        # an ensemble pipeline: (parts, K, B / parts), per sub-batch of tiles the ids of its draws, draw-major
        parts, K, h = hv["noise_ids"].shape
        tile = np.empty(B, np.int64)
        tile[:m] = params["noise_ids"][a:b]
        tile[m:] = tile[m - 1]
        hv["noise_ids"][...] = PG.ensemble_noise_ids(tile, K).reshape(K, parts, h).transpose(1, 0, 2)
    elif "noise_ids" in params:                   # (a pipeline that paints with pixel noise: _with_noise)
        hv["noise_ids"][:m] = params["noise_ids"][a:b]
        hv["noise_org"][:m] = params["noise_org"][a:b]
        keys += ("noise_ids", "noise_org")
    if m < B:                                     # a short last batch: pad with its last tile's parameters
        for k in keys:
            hv[k][m:] = hv[k][m - 1]


def _with_noise(params, noise_ids, noise_origins, N, H, W, lo, hi):
    """``params`` of tiles [lo, hi) of ``N`` with the two fields of a pipeline that paints with pixel noise:
    ``noise_ids`` / ``noise_org`` of all N tiles, checked (``paint_graph.noise_lattice``: ValueError), cut to [lo, hi)."""
    ids, org = PG.noise_lattice(noise_ids, noise_origins, N, H, W)
    if org is None:
        org = np.zeros((N, 2), np.int32)
    return dict(params, noise_ids=ids[lo:hi], noise_org=org[lo:hi])


def _paint_graph(model, B, scales, modes, pixel_noise=False, ensemble=None):
    """``model.paint_graph(B)`` with the keywords only a CVAE's takes, where they say something."""
    kw = {k: v for k, v in (("scales", scales), ("modes", modes), ("pixel_noise", pixel_noise or None)) if v is not None}
    return model.paint_graph(B, **kw, **(ensemble or {}))


def _n_fields(modes):
    """The number of label fields ``modes`` speaks of: (input mode, (mode of field 0, ...)) for several, 1 otherwise."""
    return len(modes[1]) if modes is not None and isinstance(modes[1], (tuple, list)) else 1


def _paint_stream_pipeline(painter, model, inputs, tile_shape, lo, hi, B, params, ids, seed, out, scales=None,
                           modes=None, ensemble=None):
    """Tiles [lo, hi) of ``inputs`` through ``model.paint_graph(B)``: pinned double-buffered upload / replay / download
    (``CVAEPainter.paint_stream``).  ``params`` and ``ids`` hold those tiles only.  Returns the (hi - lo, H, W) float32
    result (``out`` if given).  ``scales``: a multi-scale CVAE painter's split-scale description (``CVAE.paint_graph``);
    raw tiles and painted tiles are single-channel either way.  ``modes``: a CVAE painter's (input, label)
    range-compression modes where they are not both shift-log (``CVAE.paint_graph``), or (input mode, (mode of field 0,
    ...)) of a painter with F > 1 label fields: the result, the slots' ``out`` and the pinned output buffers are then
    (.., F, H, W), and ``out``, where given, must have the result's shape.  ``ensemble`` = {"draws": K,
    "return_draws": bool} (``CVAEPainter.paint_ensemble``; ``out`` is None): ``B`` TILES per batch through
    ``model.paint_graph(B, draws=K)``, whose slots have ``mean`` and ``var`` (and ``draws``) in place of ``out``; the
    result is the tuple of these, (hi - lo, [F,] H, W) and (hi - lo, K, [F,] H, W) NumPy arrays."""
    H, W = tile_shape
    dev = model.device
    F = _n_fields(modes)
    field = (F,) if F > 1 else ()
    shape = (hi - lo, *field, H, W)
    if F > 1 and out is not None and tuple(out.shape) != shape:
        raise ValueError(f"out must have the shape {shape} of {F} label fields, got {tuple(out.shape)}")
    g = _paint_graph(model, B, scales, modes, "noise_ids" in params, ensemble)
    torch_in = isinstance(inputs, torch.Tensor)
    # what leaves a slot: name -> (shape of a tile in the slot, the result it lands in)
    if ensemble is None:
        result = out if out is not None else np.empty(shape, np.float32)
        outs = {"out": ((F, H, W), result)}
    else:
        K = ensemble["draws"]
        outs = {"mean": ((F, H, W), np.empty(shape, np.float32)), "var": ((F, H, W), np.empty(shape, np.float32))}
        if ensemble["return_draws"]:
            outs["draws"] = ((K, F, H, W), np.empty((hi - lo, K, *field, H, W), np.float32))
        result = tuple(res for _, res in outs.values())
    torch_out = isinstance(out, torch.Tensor)
    main = torch.cuda.current_stream(dev)
    up, down = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    # Two slots = the graph's own two buffer sets (paint_graph): uploads land where the load kernel reads, downloads
    # leave from where the store kernel writes.  Per slot one pinned parameter block (one copy per batch).
    block = g["param_block"]
    # pinned host buffers are kept between calls (page-locking 4 x 64 MiB costs tens of milliseconds per call);
    # release_paint_buffers() frees them; the tile buffers are only allocated for NumPy inputs / outputs
    cache = painter.__dict__.setdefault("_paint_host_buffers", {})
    key = (B, H, W, g["block_bytes"], str(dev)) + ((F,) if F > 1 else ())
    if ensemble is not None:
        key = ("ensemble", K, "draws" in outs) + key
    if key not in cache:
        cache.clear()
        cache[key] = [{"h_blk": torch.zeros(g["block_bytes"], dtype=torch.uint8).pin_memory(), "h_in": None,
                       "h_out": None} for _ in range(2)]
    slots = []
    for gs, hb in zip(g["slots"], cache[key]):
        h_blk = hb["h_blk"]
        hv = block.views(h_blk)
        hv["seed"][0] = PG.seed_word(seed)
        if not torch_in and hb["h_in"] is None:
            hb["h_in"] = torch.empty((B, 1, H, W), dtype=torch.float32).pin_memory()
        if not torch_out and hb["h_out"] is None:
            hb["h_out"] = {name: torch.empty((B, *tile), dtype=torch.float32).pin_memory()
                           for name, (tile, _) in outs.items()}
        slots.append({"g": gs, "h_blk": h_blk, "hv": hv, "h_in": hb["h_in"], "h_out": hb["h_out"],
                      "ev_up": torch.cuda.Event(), "ev_done": torch.cuda.Event(), "ev_down": torch.cuda.Event(),
                      "pending": None})

    def harvest(sl):
        if sl["pending"] is None:
            return
        a, b = sl["pending"]
        sl["ev_down"].synchronize()
        if not torch_out:
            for name, (_, res) in outs.items():
                res[a - lo:b - lo] = sl["h_out"][name][:b - a].numpy().reshape(b - a, *res.shape[1:])
        sl["pending"] = None

    starts = list(range(lo, hi, B))

    def upload(bi):
        """Fill slot bi % 2's pinned buffers with batch bi and start its host-to-device copies."""
        a = starts[bi]
        b = min(a + B, hi)
        m = b - a
        sl = slots[bi % 2]
        gs = sl["g"]
        sl["ev_up"].synchronize()                     # the slot's previous upload has left its pinned buffers
        _fill_block(sl["hv"], params, ids, a - lo, b - lo, B)
        if torch_in:
            src = inputs[a:b].reshape(m, 1, H, W)
        else:
            sl["h_in"][:m, 0].numpy()[...] = np.asarray(inputs[a:b], dtype=np.float32)
            src = sl["h_in"][:m]
        up.wait_event(sl["ev_done"])                  # the slot's previous batch has been painted (inputs read)
        with torch.cuda.stream(up):
            gs["raw"][:m].copy_(src, non_blocking=True)
            gs["block"].copy_(sl["h_blk"], non_blocking=True)
            sl["ev_up"].record(up)

    with torch.no_grad():
        if starts:
            upload(0)
        for bi, a in enumerate(starts):
            b = min(a + B, hi)
            m = b - a
            sl = slots[bi % 2]
            gs = sl["g"]
            # The NEXT batch's upload is enqueued BEFORE this batch's graph: copies enqueued behind a graph launch
            # only start once that graph has drained (measured: tools/paint_probe.py -- the upload then sits on the
            # critical path, 1.2 ms per 64 tiles); enqueued ahead of it they run beside it.
            if bi + 1 < len(starts):
                upload(bi + 1)
            harvest(sl)                                   # this slot's previous batch has left the device
            main.wait_event(sl["ev_up"])
            main.wait_event(sl["ev_down"])                # ... and its previous output has been downloaded
            gs["graph"].replay()
            sl["ev_done"].record(main)
            down.wait_event(sl["ev_done"])
            with torch.cuda.stream(down):
                for name in outs:
                    dst = result[a - lo:b - lo].reshape(m, F, H, W) if torch_out else sl["h_out"][name][:m]
                    dst.copy_(gs[name][:m], non_blocking=True)
                sl["ev_down"].record(down)
            sl["pending"] = (a, b)
        for sl in slots:
            harvest(sl)
        torch.cuda.synchronize(dev)
    return result


class TileKeep:
    """The device side of a ``lightcone.TileReport``, for one plane or for all tiled planes of a light cone: ``cap``
    slots for problematic tiles -- index, raw (tile, tile) and painted (F, tile, tile) float32 -- behind ONE int32
    cursor in device memory that ``bp_tile_keep`` advances batch after batch, plane after plane, on the painter's
    stream, and per plane the (n_tiles * F) counts and statistics ``bp_tile_outliers`` leaves.  Nothing is read back
    before ``download()``."""

    def __init__(self, painter, tile, cap, regularise_std):
        dev = painter.model.device
        self.F = len(getattr(painter, "label_fields", None) or [None])
        self.tile, self.cap, self.regularise_std = int(tile), int(cap), float(regularise_std)
        slots = max(self.cap, 1)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.index = torch.full((slots,), -1, dtype=torch.int32, device=dev)
        self.raw = torch.empty((slots, self.tile, self.tile), dtype=torch.float32, device=dev)
        self.painted = torch.empty((slots, self.F, self.tile, self.tile), dtype=torch.float32, device=dev)
        self.planes = []

    def plane(self, first_index, n_tiles, n_side, first_tile_id, z, number=None):
        """The record of the next plane: its tiles take the slot indices ``first_index`` ... + ``n_tiles``."""
        dev = self.cursor.device
        rec = {"keep": self, "first_index": int(first_index), "n_tiles": int(n_tiles), "n_side": int(n_side),
               "first_tile_id": int(first_tile_id), "z": z, "plane": number,
               "counts": torch.empty(n_tiles * self.F, dtype=torch.int32, device=dev),
               "stats": torch.empty(2 * n_tiles * self.F, dtype=torch.float64, device=dev)}
        self.planes.append(rec)
        return rec

    def download(self):
        """One synchronising download.  Per plane, in the order painted: (record, mean, std, n_outliers -- (n_tiles, F)
        -- and of its kept tiles the tile numbers, the raw tiles and the paintings ((tile, tile) where F = 1))."""
        kept = min(int(self.cursor.cpu()[0]), self.cap)
        index = self.index[:kept].cpu().numpy()
        raw, painted = self.raw[:kept].cpu().numpy(), self.painted[:kept].cpu().numpy()
        if self.F == 1:
            painted = painted[:, 0]
        out = []
        for rec in self.planes:
            n, F = rec["n_tiles"], self.F
            stats = rec["stats"].cpu().numpy().reshape(n, F, 2)
            sel = np.flatnonzero((index >= rec["first_index"]) & (index < rec["first_index"] + n))
            out.append((rec, stats[..., 0].copy(), stats[..., 1].copy(), rec["counts"].cpu().numpy().reshape(n, F),
                        index[sel] - rec["first_index"], [raw[s] for s in sel], [painted[s] for s in sel]))
        return out


def _paint_plane_pipeline(painter, model, tile, delta, geo, B, params, tile_ids, seed, weight_map, regularise_std, out,
                          scales=None, modes=None, keep=None):
    """One plane through ``model.paint_graph(B)`` on the device (``CVAEPainter._paint_plane_device``): cut, parameter
    block, replay, blend per batch on ONE stream, then the division.  ``modes`` of F > 1 label fields: the slots' ``out``
    is (B, F, tile, tile), blended by ``bp_plane_blend_fields`` into one accumulator plane per field; the result (and
    ``out``) is (F, n_plane, n_plane).  ``keep``: the plane's ``TileKeep.plane`` record; between replay and blend every
    batch then runs ``bp_tile_outliers`` on the slot's ``out`` and ``bp_tile_keep`` on the slot's ``raw`` and ``out``."""
    import ctypes as C
    from . import _lib as L
    dev = model.device
    cut, n_plane = geo["cut"], geo["n_plane"]
    n = len(geo["origins"])
    F = _n_fields(modes)
    shape = (F, n_plane, n_plane) if F > 1 else (n_plane, n_plane)
    if isinstance(delta, torch.Tensor):
        if delta.device != torch.device(dev):
            raise ValueError(f"delta lives on {delta.device}, the painter on {dev}")
        d = delta if delta.is_contiguous() else delta.contiguous()
    else:
        d = torch.from_numpy(np.ascontiguousarray(delta)).to(dev)
    if d.dim() != 2 or d.dtype not in (torch.float32, torch.float64):
        raise TypeError("delta must be a 2-d float32 or float64 plane")
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != torch.device(dev) or
                            out.dtype != torch.float64 or tuple(out.shape) != shape or
                            not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float64 ({', '.join(str(v) for v in shape)}) tensor on {dev}")
    tk = keep["keep"] if keep is not None else None
    if tk is not None and (tk.F != F or tk.tile != tile or keep["n_tiles"] != n or tk.cursor.device != torch.device(dev)):
        raise ValueError(f"the tile keep is for {keep['n_tiles']} tiles of {tk.F} x {tk.tile}^2 on {tk.cursor.device}, "
                         f"the plane has {n} of {F} x {tile}^2 on {dev}")
    g = _paint_graph(model, B, scales, modes, "noise_ids" in params)
    # per-plane parameter blocks, one per batch, built like paint_stream's pinned ones and uploaded once: a batch
    # then costs one device-to-device copy of its block into the slot
    block = g["param_block"]
    n_batches = (n + B - 1) // B
    blocks = torch.zeros((n_batches, g["block_bytes"]), dtype=torch.uint8)
    for bi in range(n_batches):
        hv = block.views(blocks[bi])
        hv["seed"][0] = PG.seed_word(seed)
        _fill_block(hv, params, tile_ids, bi * B, min(bi * B + B, n), B)
    lib = L.load()
    # accumulators and the resampling scratch are kept between calls (release_paint_buffers() frees them)
    cache = painter.__dict__.setdefault("_plane_device_buffers", {})
    ws = int(lib.bp_plane_cut_workspace(B, cut, tile))
    key = (n_plane, B, ws, str(dev)) + ((F,) if F > 1 else ())
    if key not in cache:
        cache.clear()
        cache[key] = {"acc": torch.empty(shape, dtype=torch.float64, device=dev),
                      "wsum": torch.empty(shape, dtype=torch.float64, device=dev),
                      "scratch": torch.empty(max(ws // 8, 1), dtype=torch.float64, device=dev),
                      "stats": torch.empty(2 * B * F, dtype=torch.float64, device=dev)}
    buf = cache[key]
    acc, wsum = buf["acc"], buf["wsum"]
    result = out if out is not None else torch.empty(shape, dtype=torch.float64, device=dev)
    with torch.no_grad():
        blocks_d = blocks.to(dev)
        org_d = torch.from_numpy(geo["origins"]).to(dev)
        dst_d = torch.from_numpy(geo["dst"]).to(dev)
        w_d = torch.from_numpy(np.ascontiguousarray(weight_map, dtype=np.float64)).to(dev)
        acc.zero_()
        wsum.zero_()
        sm = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        dtype = L.F32 if d.dtype == torch.float32 else L.F64
        reg = regularise_std is not None
        rows, cols = d.shape
        for bi in range(n_batches):
            a, b = bi * B, min(bi * B + B, n)
            m = b - a
            gs = g["slots"][bi % 2]               # (one stream: the slots' reuse is ordered by the stream itself)
            L.check(lib.bp_plane_cut(L.ptr(d), dtype, rows, cols, C.c_void_p(org_d.data_ptr() + 8 * a), m, cut,
                                     tile, L.ptr(buf["scratch"]), ws, L.ptr(gs["raw"]), sm), "plane cut")
            gs["block"].copy_(blocks_d[bi])
            gs["graph"].replay()
            if keep is not None:
                counts = C.c_void_p(keep["counts"].data_ptr() + 4 * a * F)
                L.check(lib.bp_tile_outliers(L.ptr(gs["out"]), m * F, tile, tk.regularise_std,
                                             C.c_void_p(keep["stats"].data_ptr() + 16 * a * F), counts, sm),
                        "tile outliers")
                L.check(lib.bp_tile_keep(L.ptr(gs["raw"]), L.ptr(gs["out"]), counts, m, F, tile,
                                         keep["first_index"] + a, tk.cap, L.ptr(tk.cursor), L.ptr(tk.index),
                                         L.ptr(tk.raw), L.ptr(tk.painted), sm), "tile keep")
            box = geo["dst"][a:b]
            blend = (lib.bp_plane_blend, (m,)) if F == 1 else (lib.bp_plane_blend_fields, (m, F))
            L.check(blend[0](L.ptr(gs["out"]), *blend[1], tile, C.c_void_p(dst_d.data_ptr() + 8 * a),
                             int(box[:, 0].min()), int(box[:, 1].min()), int(box[:, 0].max()) + tile,
                             int(box[:, 1].max()) + tile, L.ptr(w_d), 1 if reg else 0,
                             float(regularise_std) if reg else 0.0, L.ptr(buf["stats"]), L.ptr(acc),
                             L.ptr(wsum), n_plane, n_plane, sm), "plane blend")
        L.check(lib.bp_plane_finish(L.ptr(acc), L.ptr(wsum), F * n_plane * n_plane, L.ptr(result), sm), "plane finish")
        if out is not None:
            return out
        return result.cpu().numpy()


def _check_moments_out(out, shape, dev):
    """``out`` of an ensemble: None, or the pair (mean, var) of two different contiguous CUDA float64 tensors of ``shape``
    on ``dev`` (ValueError)."""
    if out is None:
        return
    dev = torch.device(dev)
    if not (isinstance(out, (tuple, list)) and len(out) == 2 and
            all(isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float64 and
                tuple(t.shape) == tuple(shape) and t.is_contiguous() for t in out) and
            out[0].data_ptr() != out[1].data_ptr()):
        raise ValueError(f"out must be a pair (mean, var) of contiguous float64 ({', '.join(str(v) for v in shape)}) "
                         f"tensors on {dev}")


def _plane_moments(lib, acc, wsum, K, shape, out, planes, sm):
    """``bp_plane_moments`` on stream ``sm`` over the contiguous CUDA float64 (K, *shape) ``acc`` and ``wsum`` (None: the
    draws are ``acc`` itself, nothing is divided).  ``planes``: None, a (K, *shape) tensor that receives the K quotients,
    or ``acc`` itself where ``wsum`` is None.  Returns (mean, var[, planes]): ``out`` = (mean, var) filled, everything
    left on the device; without ``out`` NumPy arrays."""
    from . import _lib as L
    mean, var = out if out is not None else (torch.empty(shape, dtype=torch.float64, device=acc.device) for _ in range(2))
    L.check(lib.bp_plane_moments(L.ptr(acc), L.ptr(wsum), K, int(np.prod(shape)), L.ptr(mean), L.ptr(var),
                                 L.ptr(planes if planes is not acc else None), sm), "plane moments")
    res = (mean, var) + ((planes,) if planes is not None else ())
    if out is not None:
        return res
    return tuple(t.cpu().numpy() for t in res)


def _paint_plane_ensemble_pipeline(painter, model, tile, delta, geo, B, K, params, tile_ids, seed, weight_map,
                                   regularise_std, out, scales=None, modes=None, return_planes=False, moments=True):
    """The ensemble form of ``_paint_plane_pipeline`` (``lightcone.paint_plane_ensemble(on_device=True)``): one plane
    through ``model.paint_graph(B, draws=K)`` with its draws, ``B`` TILES per batch.  Per batch on ONE stream: cut,
    parameter block (the four-double records of an ensemble block), replay, and ``bp_plane_blend_fields`` with
    ``fields = K F`` over the slot's (B, K, F, tile, tile) ``draws`` into the (K, F, n_plane, n_plane) float64
    accumulators -- the bits of plane (k, f) are ``bp_plane_blend``'s on draw k's tiles of field f.  Then
    ``bp_plane_moments`` across the K planes: (mean, var[, planes]) as NumPy arrays, (n_plane, n_plane) and
    (K, n_plane, n_plane), with a leading F behind K for F > 1 label fields; or ``out`` = (mean, var), CUDA float64
    tensors, filled and returned (the planes then stay a CUDA tensor too).  ``moments=False``: the accumulators are
    divided in place (``bp_plane_finish``) and returned, a (K, [F,] n_plane, n_plane) CUDA tensor that is valid until the
    next plane of this painter is painted.

    Memory: the accumulators are ``16 K F n_plane^2`` bytes (4.3 GB at 4096^2 and K = 16, F = 1), cached beside
    ``_paint_plane_pipeline``'s until ``release_paint_buffers()``; ``return_planes`` adds ``8 K F n_plane^2``."""
    import ctypes as C
    from . import _lib as L
    dev = model.device
    cut, n_plane = geo["cut"], geo["n_plane"]
    n = len(geo["origins"])
    F = _n_fields(modes)
    field = (F,) if F > 1 else ()
    shape = (*field, n_plane, n_plane)
    if isinstance(delta, torch.Tensor):
        if delta.device != torch.device(dev):
            raise ValueError(f"delta lives on {delta.device}, the painter on {dev}")
        d = delta if delta.is_contiguous() else delta.contiguous()
    else:
        d = torch.from_numpy(np.ascontiguousarray(delta)).to(dev)
    if d.dim() != 2 or d.dtype not in (torch.float32, torch.float64):
        raise TypeError("delta must be a 2-d float32 or float64 plane")
    _check_moments_out(out, shape, dev)
    g = _paint_graph(model, B, scales, modes, False, {"draws": K, "return_draws": True})
    block = g["param_block"]
    n_batches = (n + B - 1) // B
    blocks = torch.zeros((n_batches, g["block_bytes"]), dtype=torch.uint8)
    for bi in range(n_batches):
        hv = block.views(blocks[bi])
        hv["seed"][0] = PG.seed_word(seed)
        _fill_block(hv, params, tile_ids, bi * B, min(bi * B + B, n), B)
    lib = L.load()
    # the accumulators of the K planes are kept between calls, beside _paint_plane_pipeline's buffers and in their
    # place: one large set at a time (release_paint_buffers() frees them)
    cache = painter.__dict__.setdefault("_plane_device_buffers", {})
    ws = int(lib.bp_plane_cut_workspace(B, cut, tile))
    key = ("ensemble", K, n_plane, B, ws, str(dev), F)
    if key not in cache:
        for k in [k for k in cache if k[0] != "small"]:
            del cache[k]
        cache[key] = {"acc": torch.empty((K, F, n_plane, n_plane), dtype=torch.float64, device=dev),
                      "wsum": torch.empty((K, F, n_plane, n_plane), dtype=torch.float64, device=dev),
                      "scratch": torch.empty(max(ws // 8, 1), dtype=torch.float64, device=dev),
                      "stats": torch.empty(2 * B * K * F, dtype=torch.float64, device=dev)}
    buf = cache[key]
    acc, wsum = buf["acc"], buf["wsum"]
    with torch.no_grad():
        blocks_d = blocks.to(dev)
        org_d = torch.from_numpy(geo["origins"]).to(dev)
        dst_d = torch.from_numpy(geo["dst"]).to(dev)
        w_d = torch.from_numpy(np.ascontiguousarray(weight_map, dtype=np.float64)).to(dev)
        acc.zero_()
        wsum.zero_()
        sm = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        dtype = L.F32 if d.dtype == torch.float32 else L.F64
        reg = regularise_std is not None
        rows, cols = d.shape
        for bi in range(n_batches):
            a, b = bi * B, min(bi * B + B, n)
            m = b - a
            gs = g["slots"][bi % 2]               # (one stream: the slots' reuse is ordered by the stream itself)
            L.check(lib.bp_plane_cut(L.ptr(d), dtype, rows, cols, C.c_void_p(org_d.data_ptr() + 8 * a), m, cut,
                                     tile, L.ptr(buf["scratch"]), ws, L.ptr(gs["raw"]), sm), "plane cut")
            gs["block"].copy_(blocks_d[bi])
            gs["graph"].replay()
            box = geo["dst"][a:b]
            # tile t's planes (k, f) are the K F "fields" of the blend: tiles[t * K F + k F + f] into plane k F + f
            L.check(lib.bp_plane_blend_fields(L.ptr(gs["draws"]), m, K * F, tile, C.c_void_p(dst_d.data_ptr() + 8 * a),
                                              int(box[:, 0].min()), int(box[:, 1].min()), int(box[:, 0].max()) + tile,
                                              int(box[:, 1].max()) + tile, L.ptr(w_d), 1 if reg else 0,
                                              float(regularise_std) if reg else 0.0, L.ptr(buf["stats"]), L.ptr(acc),
                                              L.ptr(wsum), n_plane, n_plane, sm), "plane blend of the draws")
        if not moments:                           # (finish_kernel reads and writes element i in one thread: in place)
            L.check(lib.bp_plane_finish(L.ptr(acc), L.ptr(wsum), K * F * n_plane * n_plane, L.ptr(acc), sm),
                    "plane finish of the draws")
            return acc.view(K, *shape)
        planes = torch.empty((K, *shape), dtype=torch.float64, device=dev) if return_planes else None
        return _plane_moments(lib, acc, wsum, K, shape, out, planes, sm)


def _paint_small_plane_pipeline(painter, model, tile, plane, origin, size, crop, params, ids, seed, subtract_minimum,
                                field_index, out, scales=None, modes=None, ensemble=None):
    """One tile through ``model.paint_graph(1)`` on the device (``Painter._paint_small_plane_device``): minimum, zoom
    into slot 0's ``raw``, parameter block, replay, crop, on ONE stream.  ``modes`` of F > 1 label fields: the slot's
    ``out`` is (1, F, tile, tile) and ``field_index`` says which field is cropped.  ``ensemble`` = (K, return_planes,
    moments): ``model.paint_graph(1, draws=K)`` with its ``draws`` (1, K, F, tile, tile), the field cropped once per draw
    into (K, m, m) float64, and ``bp_plane_moments`` without weights across them: (mean, var[, planes]) as NumPy, or
    ``out`` = (mean, var) filled (the planes then stay a CUDA tensor); ``moments`` False: the (K, m, m) CUDA tensor
    alone."""
    import ctypes as C
    from . import _lib as L
    dev = torch.device(model.device)
    F = _n_fields(modes)
    if F > 1 and (field_index is None or not 0 <= field_index < F):
        raise ValueError(f"a painter with {F} label fields needs the index of the field to crop")
    j = field_index if F > 1 else 0
    if (not isinstance(plane, torch.Tensor) or plane.device != dev or plane.dim() != 2 or not plane.is_contiguous() or
            plane.dtype not in (torch.float32, torch.float64)):
        raise TypeError(f"the plane must be a contiguous 2-d float32 or float64 tensor on {dev}")
    r0, c0, m = (int(v) for v in crop)
    if ensemble is not None:
        K = ensemble[0]
        _check_moments_out(out, (m, m), dev)
    elif out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float64 or
                              tuple(out.shape) != (m, m) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float64 ({m}, {m}) tensor on {dev}")
    g = _paint_graph(model, 1, scales, modes, "noise_ids" in params,
                     None if ensemble is None else {"draws": K, "return_draws": True})
    block = g["param_block"]
    blk = torch.zeros(g["block_bytes"], dtype=torch.uint8)
    hv = block.views(blk)
    hv["seed"][0] = PG.seed_word(seed)
    _fill_block(hv, params, ids, 0, 1, 1)
    lib = L.load()
    # the resampling scratch is kept between calls, beside _paint_plane_pipeline's (release_paint_buffers() frees it)
    cache = painter.__dict__.setdefault("_plane_device_buffers", {})
    ws, ws_min = int(lib.bp_window_zoom_workspace(size, tile)), int(lib.bp_window_min_workspace())
    key = ("small", ws, str(dev))
    if key not in cache:
        for k in [k for k in cache if k[0] == "small"]:
            del cache[k]
        cache[key] = {"scratch": torch.empty(max(ws // 8, 1), dtype=torch.float64, device=dev),
                      "min_scratch": torch.empty(ws_min // 8, dtype=torch.float64, device=dev),
                      "min": torch.empty(1, dtype=torch.float64, device=dev)}
    buf = cache[key]
    if ensemble is not None:
        result = torch.empty((K, m, m), dtype=torch.float64, device=dev)
    else:
        result = out if out is not None else torch.empty((m, m), dtype=torch.float64, device=dev)
    with torch.no_grad(), torch.cuda.device(dev):
        sm = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        dtype = L.F32 if plane.dtype == torch.float32 else L.F64
        rows, cols = plane.shape
        x0, y0 = int(origin[0]), int(origin[1])
        gs = g["slots"][0]
        minimum = None
        if subtract_minimum:
            minimum = L.ptr(buf["min"])               # (one value of the plane's dtype at the front of a double)
            L.check(lib.bp_window_min(L.ptr(plane), dtype, rows, cols, x0, y0, size, L.ptr(buf["min_scratch"]), ws_min,
                                      minimum, sm), "window min")
        L.check(lib.bp_window_zoom(L.ptr(plane), dtype, rows, cols, x0, y0, size, minimum, tile, L.ptr(buf["scratch"]),
                                   buf["scratch"].numel() * 8, L.ptr(gs["raw"]), sm), "window zoom")
        gs["block"].copy_(blk.to(dev))
        gs["graph"].replay()
        if ensemble is not None:
            for k in range(K):                        # draw k, field j of the slot's (1, K, F, tile, tile) draws
                img = C.c_void_p(gs["draws"].data_ptr() + 4 * (k * F + j) * tile * tile)
                L.check(lib.bp_tile_crop(img, tile, r0, c0, m, L.ptr(result[k]), sm), "tile crop")
            if not ensemble[2]:
                return result
            return _plane_moments(lib, result, None, K, (m, m), out, result if ensemble[1] else None, sm)
        img = C.c_void_p(gs["out"].data_ptr() + 4 * j * tile * tile)
        L.check(lib.bp_tile_crop(img, tile, r0, c0, m, L.ptr(result), sm), "tile crop")
        if out is not None:
            return out
        return result.cpu().numpy()


def dataloader_shuffle_order(n):
    """The index order ``DataLoader(dataset, shuffle=True)`` would produce next, consuming the global
    torch RNG the same way (iterator base seed first, then the RandomSampler's generator seed)."""
    torch.empty((), dtype=torch.int64).random_()                       # _BaseDataLoaderIter._base_seed
    seed = int(torch.empty((), dtype=torch.int64).random_().item())    # RandomSampler.__iter__
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g).tolist()


class _DeviceLoader:
    """Yields the same ``(fields, indices, redshifts)`` batches as the reference's DataLoader, in the
    same shuffled order, with the tiles assembled on the GPU."""

    def __init__(self, assembler, n, batch_size):
        self.asm, self.n, self.batch_size = assembler, n, batch_size

    def __iter__(self):
        order = dataloader_shuffle_order(self.n)
        for s in range(0, self.n, self.batch_size):
            idx = order[s:s + self.batch_size]
            x, y, z = self.asm.get_batch(idx)
            yield [y, x], torch.tensor(idx), z

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size


class _ShardedLoader:
    """Data-parallel replacement for ``DataLoader(shuffle=True)``: every rank draws the SAME
    global permutation (seeded, advanced per pass) and takes its slice of each global batch
    (baryon_painter_amd.dist.shard_indices), so the union over ranks is what one device would
    have processed."""

    def __init__(self, dataset, batch_size, sync, seed=20190101):
        self.dataset, self.batch_size, self.sync = dataset, batch_size, sync
        self.seed, self.epoch = seed, 0

    def __iter__(self):
        from .dist import shard_indices
        rng = np.random.Generator(np.random.PCG64([self.seed, self.epoch]))
        self.epoch += 1
        perm = rng.permutation(len(self.dataset))
        collate = torch.utils.data.default_collate
        for idx in shard_indices(perm, self.sync.rank, self.sync.world_size, self.batch_size):
            yield collate([self.dataset[int(i)] for i in idx])

    def __len__(self):
        return len(self.dataset) // (self.batch_size * self.sync.world_size)


class TrainingStats:
    """Loss log with moving average and the reference's text format (painter.py:447-545):
    header ``# Batch nr, sample nr, <labels>``, one line ``batch sample v0 v1 ...`` per push."""

    def __init__(self, loss_terms=[], moving_average_window=100, dump_to_file_frequency=10, stats_filename=None):
        self.mavg_window = moving_average_window
        self.n_batches = 0
        self.n_processed_samples = []
        self.last_dump_to_file = 0
        self.dump_to_file_frequency = dump_to_file_frequency
        self.loss_terms = collections.OrderedDict((t, {"all": [], "mavg": []}) for t in loss_terms)
        self.stats_filename = stats_filename
        if stats_filename is not None:
            with open(stats_filename, "w") as f:
                f.write("# Batch nr, sample nr, {}\n".format(", ".join(loss_terms)))

    def __del__(self):
        try:
            self.flush_to_file()
        except Exception:
            pass

    def push_loss(self, n_sample, *args):
        self.n_batches += 1
        self.n_processed_samples.append(n_sample)
        for value, term in zip(args, self.loss_terms.values()):
            term["all"].append(value)
            term["mavg"].append(np.mean(term["all"][-min(self.n_batches, self.mavg_window):]))
        if self.stats_filename is not None and self.n_batches - self.dump_to_file_frequency >= self.last_dump_to_file:
            self.flush_to_file()

    def flush_to_file(self):
        if self.stats_filename is None:
            return
        with open(self.stats_filename, "a") as f:
            for s in range(self.last_dump_to_file, self.n_batches):
                f.write(self.get_str(s) + "\n")
        self.last_dump_to_file = self.n_batches

    def get_str(self, idx=-1):
        batch = idx if idx >= 0 else self.n_batches + idx + 1
        return f"{batch} {self.n_processed_samples[idx]} " + "".join(f"{t['all'][idx]} " for t in self.loss_terms.values())

    def get_pretty_str(self, n_col=1):
        width = max(len(k) for k in self.loss_terms)
        out, in_row = "", 0
        for key, term in self.loss_terms.items():
            out += "{key:<{width}s}: {value:8.3e}     ".format(key=key, width=width, value=term["mavg"][-1])
            in_row += 1
            if in_row >= n_col:
                out += "\n"
                in_row = 0
        return out


class CGANPainter(Painter):
    """Painter around the conditional GAN (models/cgan.py) with the ``paint`` keywords of the
    reference's external ``GAN_Painter`` (scripts/create_lightcone.py:47-54,
    process_SLICS.py:170-172).  Field transform: the reference's CGAN used a "shift-log-cam" map into
    the tanh range (trained_models/CGAN/fiducial/transform.pickle: log(x/sigma+1)/k0 - k1 with
    k = [4, 1]); it is applied here on top of the dataset's statistics.

    ``paint_batch`` / ``paint_stream`` / ``_paint_plane_device`` have ``CVAEPainter``'s signatures, so every
    ``lightcone`` entry point takes either painter.  The generator has no latent noise: ``seed`` and ``tile_ids`` are
    accepted and do not affect the result.

    ``filename``: a state-dict path (the model is built from ``tile_size`` / ``n_res``; the painter has no statistics
    and cannot transform until ``stats`` is set) or a ``(state, meta)`` pair as written by
    ``save_state_to_file((state, meta))``: the model is built from the pair's ``tile_size`` / ``n_res`` and the painter
    transforms with its statistics."""

    K = (4.0, 1.0)
    META_KEYS = ("stats", "K", "tile_size", "n_res", "input_field", "label_fields", "paint_dtype",
                 "train_dtype")
    OPTIONAL_META = {"paint_dtype": "fp32", "train_dtype": "fp32"}          # keys a checkpoint written before they existed lacks: their meaning there

    def __init__(self, training_data_set=None, tile_size=512, compute_device="cuda:0", n_res=9, filename=None,
                 paint_dtype="fp32", train_dtype="fp32"):
        """``paint_dtype`` / ``train_dtype``: "fp32" or "bf16", the arithmetic of the generator's 128-channel trunk when
        painting / of its residual blocks when training (models/cgan.py); a ``(state, meta)`` checkpoint brings its own."""
        from .models.cgan import CGAN
        self.compute_device = compute_device
        self.training_data = training_data_set
        self.stats = None if training_data_set is None else training_data_set.stats
        self.input_field, self.label_fields = "dm", ["pressure"]
        self.tile_size, self.n_res = tile_size, n_res
        self.paint_dtype, self.train_dtype = paint_dtype, train_dtype
        if isinstance(filename, (tuple, list)):
            self._apply_meta(self._read_meta(filename[1]))          # (the model's geometry comes from the checkpoint)
        self.model = CGAN(tile_size=self.tile_size, device=compute_device, n_res=self.n_res, paint_dtype=self.paint_dtype,
                          train_dtype=self.train_dtype)
        if filename is not None:
            self.load_state_from_file(filename, compute_device)

    # ---- the CGAN's own field transform
    def _sigma(self, field, z):
        from .utils.data_transforms import interpolate_z
        return float(np.sqrt(interpolate_z(self.stats[field], z)["var"]))

    def transform(self, x, field, z):
        return (np.log(np.asarray(x, np.float64) / self._sigma(field, z) + 1) / self.K[0] - self.K[1]).astype(np.float32)

    def inverse_transform(self, y, field, z):
        return (np.exp((np.asarray(y, np.float64) + self.K[1]) * self.K[0]) - 1) * self._sigma(field, z)

    def train(self, n_iter=1000, batch_size=6, learning_rate=5e-5, lr_decay=0.85, lr_decay_every=1568, verbose=False):
        """Alternating D / G iterations (README.md:97,130-139): Adam(betas=(0.5, 0.999)), lr x0.85 every
        1568 iterations, batch 6.  Returns the list of loss dicts."""
        if self.training_data is None:
            raise RuntimeError("Trying to train but no training data specified.")
        m = self.model
        m.train(True)
        opt_g = torch.optim.Adam(m.g_parameters(), lr=learning_rate, betas=(0.5, 0.999))
        opt_d = torch.optim.Adam(m.d_parameters(), lr=learning_rate, betas=(0.5, 0.999))
        sched = [torch.optim.lr_scheduler.StepLR(o, step_size=lr_decay_every, gamma=lr_decay) for o in (opt_g, opt_d)]
        ds, log = self.training_data, []
        rng = np.random.default_rng(0)
        asm = getattr(self, "device_assembler", None)
        pending = []                                 # device path: loss dicts still on the device
        for it in range(n_iter):
            idx = rng.integers(0, len(ds), batch_size)
            if asm is not None:                      # index arithmetic and launches only: nothing waits for the device
                cam, aux = self._cam_rows([ds.sample_idx_to_redshift(int(i)) for i in idx])
                pending.append(m.train_step_assembled(lambda plan: asm.gather_gan(idx, cam, aux, plan), batch_size,
                                                      opt_g, opt_d))
                for s in sched:
                    s.step()
                if it == n_iter - 1 or (verbose and it % 50 == 0):
                    log.extend(self._download_losses(pending))
                    pending = []
                    if verbose and it % 50 == 0:
                        print(it, log[-1])
                continue
            dm, pr, zs = [], [], []
            for i in idx:
                d, p, z = ds.raw_fields(int(i)) if hasattr(ds, "raw_fields") else self._raw(ds, int(i))
                dm.append(self.transform(d, "dm", z)[None])
                pr.append(self.transform(p, "pressure", z)[None])
                zs.append(z)
            losses = m.train_step(torch.from_numpy(np.stack(pr)), torch.from_numpy(np.stack(dm)),
                                  torch.tensor(zs, dtype=torch.float32), opt_g, opt_d)
            for s in sched:
                s.step()
            log.append({k: float(v) for k, v in losses.items()})
            if verbose and it % 50 == 0:
                print(it, log[-1])
        return log

    @staticmethod
    def _raw(ds, i):
        z = ds.sample_idx_to_redshift(i)
        return ds.get_input_sample(i, transform=False), ds.get_label_sample(i, transform=False)[0], z

    # ---- training batches assembled on the device
    def use_device_assembly(self):
        """Keep the training stacks in HBM and let ``train`` assemble every batch there: one ``bp_gather_tiles_gan`` launch
        per iteration cuts, permutes, adds, scales and transforms the tiles of both fields and writes them straight into
        the training plan's inputs (utils.datasets.DeviceTileAssembler.gather_gan, CGAN.train_step_assembled), and the
        loop never waits for the device.  Same index sequence, optimisers, schedulers and log as the host loop.
        NotImplementedError, before anything is uploaded, for a training set without slab stacks (``SyntheticTileDataset``
        makes its tiles on the host)."""
        ds = self.training_data
        if ds is None:
            raise RuntimeError("use_device_assembly needs a training set")
        need = ("data", "sample_idx_to_tile", "sample_idx_to_tile_permutation", "apply_tile_permutation")
        if not all(hasattr(ds, a) for a in need):
            raise NotImplementedError(f"{type(ds).__name__} has no slab stacks to keep in HBM: the device assembly "
                                      "serves BAHAMASDataset-like training sets")
        if ds.input_field != self.input_field or list(ds.label_fields)[:1] != self.label_fields:
            raise NotImplementedError(f"the CGAN trains on {self.input_field} -> {self.label_fields[0]}; the training set "
                                      f"holds {ds.input_field} -> {list(ds.label_fields)}")
        self.device_assembler = datasets.DeviceTileAssembler(ds, self.compute_device, mode=None)

    def _cam_rows(self, zs):
        """(cam (n, 2, 3) float64, aux (n,) float32) of ``bp_gather_tiles_gan`` for samples at redshifts ``zs``:
        {sigma, k0, k1} of the input and of the label field with the sigma ``transform`` divides by, and z - 1 in float32
        as ``CGAN._inputs`` forms it.  One row per redshift is computed once."""
        memo = self.__dict__.setdefault("_cam_memo", {})
        for z in zs:
            if z not in memo:
                memo[z] = [[self._sigma(f, z), self.K[0], self.K[1]] for f in (self.input_field, self.label_fields[0])]
        return (np.array([memo[z] for z in zs], np.float64),
                np.asarray(zs, np.float64).astype(np.float32) - np.float32(1.0))

    @staticmethod
    def _download_losses(pending):
        """Loss dicts of device scalars -> dicts of floats, in one download."""
        if not pending:
            return []
        keys = list(pending[0])
        vals = torch.stack([d[k] for d in pending for k in keys]).cpu().tolist()
        return [dict(zip(keys, vals[i * len(keys):(i + 1) * len(keys)])) for i in range(len(pending))]

    # ------------------------------------------------------------------------------ inference
    def paint(self, input, z=0.0, transform=True, inverse_transform=True, pixel_noise=False):
        """``pixel_noise=True`` is a ValueError: the generator has no likelihood to draw from."""
        if pixel_noise:
            self._need_pixel_noise()
        self.model.train(False)
        y = self.transform(input, "dm", z) if transform else np.asarray(input, np.float32)
        t = self.model.tile_size
        if y.shape != (t, t):
            raise ValueError(f"Shape mismatch between input and model: {np.shape(input)} vs {(1, t, t)}")
        pred = self.model.generate(torch.from_numpy(y.reshape(1, 1, t, t)), torch.tensor([z])).cpu().numpy()
        if inverse_transform:
            return self.inverse_transform(pred[0, 0], "pressure", z)
        return pred

    def paint_batch(self, inputs, z, transform=True, inverse_transform=True, batch_size=64, use_graph=True,
                    pixel_noise=False):
        """Throughput form of ``paint``: many tiles (N, H, W) with redshifts (N,) or one, in batches through the same
        eval-mode forward, with the host transforms of ``paint``.  Returns (N, H, W) float64 physical tiles, or the
        (N, 1, H, W) float32 network output with ``inverse_transform=False``.  ``use_graph`` is accepted for
        ``CVAEPainter.paint_batch``'s signature and has no effect: this forward is launched eagerly (the graph-captured
        form is ``paint_stream``).  ``pixel_noise=True`` is a ValueError, as in ``paint``."""
        if pixel_noise:
            self._need_pixel_noise()
        self.model.train(False)
        inputs = np.asarray(inputs)
        t = self.model.tile_size
        if inputs.ndim != 3 or inputs.shape[1:] != (t, t):
            raise ValueError(f"Shape mismatch between input and model: {inputs.shape} vs {(1, t, t)}")
        zs = np.broadcast_to(np.asarray(z, dtype=np.float64), (inputs.shape[0],))
        out = []
        for s in range(0, inputs.shape[0], batch_size):
            chunk, zc = inputs[s:s + batch_size], zs[s:s + batch_size]
            if transform:
                y = np.stack([self.transform(x, "dm", float(zz)) for x, zz in zip(chunk, zc)])
            else:
                y = np.asarray(chunk, np.float32)
            pred = self.model.generate(torch.from_numpy(np.ascontiguousarray(y).reshape(-1, 1, t, t)),
                                       torch.tensor(zc, dtype=torch.float32)).cpu().numpy()
            if inverse_transform:
                pred = np.stack([self.inverse_transform(p[0], "pressure", float(zz)) for p, zz in zip(pred, zc)])
            out.append(pred)
        if not out:
            return np.empty((0, t, t)) if inverse_transform else np.empty((0, 1, t, t), np.float32)
        return np.concatenate(out, axis=0)

    def can_paint_stream(self, z=0.0):
        """Whether ``paint_stream`` can run: the painter has the statistics of both fields (a painter restored from a
        bare state dict has none).  No side effects."""
        st = self.stats
        return st is not None and all(f in st and len(st[f]) > 0 for f in (self.input_field, self.label_fields[0]))

    def _cam_parameters(self, zs):
        """``params`` of the shared pipelines for tiles at redshifts ``zs``: the rows {sigma, k0, k1} / {k0, k1, sigma}
        of the device transforms and the conditioning plane z - 1 as ``CGAN._inputs`` computes it, in float32."""
        from .utils.data_transforms import interpolate_z_many
        if not self.can_paint_stream():
            raise NotImplementedError("paint_stream needs the statistics of both fields (CGANPainter.stats; a "
                                      "(state, meta) checkpoint carries them)")
        s_in = np.sqrt(interpolate_z_many(self.stats[self.input_field], zs, "var"))
        s_out = np.sqrt(interpolate_z_many(self.stats[self.label_fields[0]], zs, "var"))
        k0, k1 = np.full_like(s_in, self.K[0]), np.full_like(s_in, self.K[1])
        return {"xf_in": np.stack([s_in, k0, k1], axis=1), "xf_out": np.stack([k0, k1, s_out], axis=1),
                "aux": np.asarray(zs, np.float64).astype(np.float32) - np.float32(1.0)}

    def _tile_shape(self):
        return self.model.tile_size, self.model.tile_size

    def _shape_mismatch(self, shape):
        return f"Shape mismatch between input and model: {shape} vs {(1, *self._tile_shape())}"

    def _device_paint_parameters(self, zs):
        """The shift-log-cam transform, the conditioning plane, the generator's tanh and the inverse transform run on the
        device (``bp_paint_load_cam`` / ``bp_paint_store_cam`` around the generator, one captured hipGraph per batch size
        on one stream); ``tile_ids`` and ``seed`` do not affect the result (no latent noise)."""
        return self._cam_parameters(zs), None, None

    def release_paint_buffers(self):
        """``Painter.release_paint_buffers``, and the model's inference plans and captured graphs."""
        super().release_paint_buffers()
        self.model.release_paint_buffers()

    # ------------------------------------------------------------------------------ checkpoints
    def _meta(self):
        """What a painter needs besides the state dict to paint in another process."""
        return {"stats": self.stats, "K": tuple(self.K), "tile_size": self.tile_size, "n_res": self.n_res,
                "input_field": self.input_field, "label_fields": list(self.label_fields),
                "paint_dtype": getattr(self, "paint_dtype", "fp32"), "train_dtype": getattr(self, "train_dtype", "fp32")}

    def _apply_meta(self, d):
        missing = [k for k in self.META_KEYS if k not in d and k not in self.OPTIONAL_META]
        if missing:
            raise ValueError(f"CGAN checkpoint metadata lacks {missing}")
        self.stats, self.K = d["stats"], tuple(d["K"])
        self.tile_size, self.n_res = d["tile_size"], d["n_res"]
        self.input_field, self.label_fields = d["input_field"], list(d["label_fields"])
        self.paint_dtype = d.get("paint_dtype", self.OPTIONAL_META["paint_dtype"])
        if self.paint_dtype not in ("fp32", "bf16"):
            raise ValueError(f"CGAN checkpoint metadata: paint_dtype {self.paint_dtype!r}")
        self.train_dtype = d.get("train_dtype", self.OPTIONAL_META["train_dtype"])
        if self.train_dtype not in ("fp32", "bf16"):
            raise ValueError(f"CGAN checkpoint metadata: train_dtype {self.train_dtype!r}")

    @staticmethod
    def _read_meta(path):
        with open(path, "rb") as f:
            return _pickler.load(f)

    def save_state_to_file(self, filename):
        """``filename``: one path -> the state dict alone; ``(state_path, meta_path)`` -> the state dict plus the
        pickled ``_meta()``, from which ``CGANPainter(filename=(state_path, meta_path))`` paints."""
        state = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        if isinstance(filename, (tuple, list)):
            with open(filename[1], "wb") as f:
                _pickler.dump(self._meta(), f)
            filename = filename[0]
        torch.save(state, filename)

    def load_state_from_file(self, filename, compute_device="cuda:0"):
        if isinstance(filename, (tuple, list)):
            d = self._read_meta(filename[1])
            if (d.get("tile_size"), d.get("n_res")) != (self.model.tile_size, self.n_res):
                raise ValueError(f"checkpoint is a {d.get('tile_size')}^2 / {d.get('n_res')}-block CGAN, this painter's "
                                 f"model a {self.model.tile_size}^2 / {self.n_res}-block one")
            self._apply_meta(d)
            self.model.paint_dtype = self.paint_dtype          # (the inference plans are cached per dtype)
            self.model.train_dtype = self.train_dtype          # (... and the training plans)
            filename = filename[0]
        self.model.load_state_dict(torch.load(filename, map_location=torch.device(compute_device)))
