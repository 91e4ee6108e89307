"""Host: the noise lattice of ``bp_likelihood_draw`` as the oracle's Philox gives it, the block layout of a paint
pipeline with pixel noise, and the checks the Python side owes the kernel.  No GPU."""
import numpy as np
import pytest
import torch

from baryon_painter_amd.models import paint_graph as PG
from oracle.philox import tile_normals

import pixel_noise_ref as R


def test_lattice_normals_are_standard_shared_on_the_lattice_and_apart_from_the_latent_draws():
    e = R.lattice_normals(5, [7, 7, 2 ** 33 + 5], [(0, 0), (5, 6), (0, 0)], 64, 64, 5)
    assert e.shape == (3, 64, 64, 5) and e.dtype == np.float32 and np.isfinite(e).all()
    print("mean", e.mean(), "std", e.std())
    assert abs(e.mean()) < 0.02 and abs(e.std() - 1) < 0.02
    # two windows of one lattice agree on their common pixels, bit for bit; another lattice differs
    assert np.array_equal(e[0, 5:, 6:].view(np.uint32), e[1, :59, :58].view(np.uint32))
    assert not np.array_equal(e[0], e[1]) and not np.array_equal(e[2], e[0])
    assert (e[2] == e[0]).mean() < 1e-3
    # bit 31 of counter word 1 keeps the lattice apart from the latent draws of the same key and id
    latent = tile_normals(5, [7], 256)
    assert np.intersect1d(e[:2].ravel().view(np.uint32), latent.ravel().view(np.uint32)).size == 0
    assert np.array_equal(R.lattice_normals(5, [7], None, 8, 8, 5), e[:1, :8, :8])


def test_paint_fields_keep_their_layout_and_gain_two_fields_with_noise():
    n, w = 6, 4
    plain = PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8))
    assert list(plain.layout) == ["xf_in", "xf_out", "tile_ids", "seed", "aux"]
    assert plain.layout == {"xf_in": (0, torch.float64, (n, w)), "xf_out": (192, torch.float64, (n, 8)),
                            "tile_ids": (576, torch.int64, (n,)), "seed": (624, torch.int64, (1,)),
                            "aux": (632, torch.float32, (n, 1))}
    assert plain.nbytes == 656
    assert PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8, noise=False)).layout == plain.layout
    noisy = PG.ParamBlock(PG.paint_fields(n, w, 1, xf_out_width=8, noise=True))
    assert list(noisy.layout) == list(plain.layout) + ["noise_ids", "noise_org"]
    assert all(noisy.layout[k] == plain.layout[k] for k in plain.layout)
    assert noisy.layout["noise_ids"] == (656, torch.int64, (n,))
    assert noisy.layout["noise_org"] == (704, torch.int32, (n, 2))
    assert noisy.nbytes == 752 and all(off % 8 == 0 for off, _, _ in noisy.layout.values())
    hv = noisy.views(torch.zeros(noisy.nbytes, dtype=torch.uint8))
    assert hv["noise_ids"].dtype == np.int64 and hv["noise_org"].shape == (n, 2) and hv["noise_org"].dtype == np.int32
    # an odd batch: the (n, 2) int32 field is a multiple of 8 bytes, the float32 aux is padded
    odd = PG.ParamBlock(PG.paint_fields(3, 2, noise=True))
    assert odd.layout["noise_ids"][0] % 8 == 0 and odd.layout["noise_org"][0] == odd.layout["noise_ids"][0] + 24
    assert odd.nbytes == odd.layout["noise_org"][0] + 24


def test_fill_block_fills_and_pads_the_noise_fields():
    from baryon_painter_amd.painter import _fill_block, _with_noise
    B, N = 4, 6
    block = PG.ParamBlock(PG.paint_fields(B, 2, noise=True))
    hv = block.views(torch.zeros(block.nbytes, dtype=torch.uint8))
    params = {"xf_in": np.arange(2.0 * N).reshape(N, 2), "xf_out": np.arange(2.0 * N).reshape(N, 2) + 100,
              "aux": np.arange(N) * 0.5}
    org = np.stack([np.arange(N) * 3, np.arange(N) * 5], axis=1)
    noisy = _with_noise(params, np.arange(N) + 2 ** 40, org, N, 64, 64, 0, N)
    assert "noise_ids" not in params and noisy["noise_org"].dtype == np.int32
    ids = np.arange(N, dtype=np.int64) + 10
    _fill_block(hv, noisy, ids, 4, 6, B)                         # a short batch: tiles 4 and 5, two rows of padding
    assert hv["noise_ids"].tolist() == [2 ** 40 + 4, 2 ** 40 + 5, 2 ** 40 + 5, 2 ** 40 + 5]
    assert hv["noise_org"].tolist() == [[12, 20], [15, 25], [15, 25], [15, 25]]
    assert hv["tile_ids"].tolist() == [14, 15, 15, 15]
    # default origins are zero; a rank's share is cut out of the checked whole
    part = _with_noise(params, np.arange(N), None, N, 64, 64, 2, 5)
    assert part["noise_ids"].tolist() == [2, 3, 4] and not part["noise_org"].any() and part["noise_org"].shape == (3, 2)
    # a block without the fields is filled as before
    plain = PG.ParamBlock(PG.paint_fields(B, 2))
    hp = plain.views(torch.zeros(plain.nbytes, dtype=torch.uint8))
    _fill_block(hp, params, ids, 0, 4, B)
    assert hp["tile_ids"].tolist() == [10, 11, 12, 13] and set(hp) == {"xf_in", "xf_out", "tile_ids", "seed", "aux"}


def test_the_lattice_limits_are_checked_on_the_host():
    ids, org = PG.noise_lattice([1, 2], [(0, 0), (2 ** 31 - 64, 2 ** 24 - 64)], 2, 64, 64)
    assert ids.dtype == np.int64 and org.dtype == np.int32 and org.tolist() == [[0, 0], [2 ** 31 - 64, 2 ** 24 - 64]]
    assert PG.noise_lattice(np.array([2 ** 63 + 1, 0], np.uint64), None, 2, 8, 8)[1] is None
    for bad in ([(0, 0), (-1, 0)], [(0, 0), (0, 2 ** 24 - 63)], [(2 ** 31 - 63, 0), (0, 0)], [(0, 0)], [(0.5, 0), (0, 0)]):
        with pytest.raises(ValueError):
            PG.noise_lattice([1, 2], bad, 2, 64, 64)
    with pytest.raises(ValueError):
        PG.noise_lattice([1, 2, 3], None, 2, 64, 64)
    with pytest.raises(ValueError):
        PG.noise_lattice([1.0, 2.0], None, 2, 64, 64)
    assert int(PG.seed_word(2 ** 63 + 5)) == 2 ** 63 + 5 - 2 ** 64 and int(PG.seed_word(-1)) == -1
