"""noahmp_amd/tile.py: the inverse of a sort permutation and the index plane of a window around the tile, against restatements written
here (torch CPU tensors, no engine); the gather of tile-order planes into a column order and back on the device."""
import numpy as np
import pytest
import torch

from noahmp_amd import tile

# (ni, nj, (nj_w, ni_w), origin (i0, j0))
SHAPES = [(1, 1, (1, 1), (0, 0)), (3, 2, (2, 3), (0, 0)), (3, 2, (5, 7), (0, 0)), (3, 2, (5, 7), (2, 1)), (3, 2, (5, 7), (4, 3))]
FIXED = {1: [0], 6: [4, 0, 5, 2, 1, 3]}


def perms(n):
    return {"none": None, "reversed": np.arange(n - 1, -1, -1, dtype=np.int32), "fixed": np.array(FIXED[n], np.int32)}


def np_inverse(perm):
    inv = np.empty(perm.size, np.int32)
    inv[perm] = np.arange(perm.size, dtype=np.int32)
    return inv


def np_window_index(shape, origin, ni, nj, pos, fill):
    want = np.full(shape, fill, np.int32)
    want[origin[1]:origin[1] + nj, origin[0]:origin[0] + ni] = (np.arange(ni * nj, dtype=np.int32) if pos is None else pos).reshape(nj, ni)
    return want


@pytest.mark.parametrize("ni, nj, shape, origin", SHAPES)
@pytest.mark.parametrize("fill", (-1, -2))
@pytest.mark.parametrize("which", ("none", "reversed", "fixed"))
def test_window_index(ni, nj, shape, origin, fill, which):
    perm = perms(ni * nj)[which]
    pos = None if perm is None else np_inverse(perm)
    got = tile.window_index(shape, origin, ni, nj, pos=None if pos is None else torch.from_numpy(pos), fill=fill)
    assert got.dtype == torch.int32 and got.is_contiguous() and tuple(got.shape) == shape
    assert np.array_equal(got.numpy(), np_window_index(shape, origin, ni, nj, pos, fill))


@pytest.mark.parametrize("n", (1, 6))
def test_inverse_perm(n):
    for perm in list(perms(n).values())[1:]:
        p = torch.from_numpy(perm)
        inv = tile.inverse_perm(p)
        assert inv.dtype == torch.int32 and inv.device == p.device
        assert np.array_equal(inv.numpy(), np_inverse(perm))
        assert np.array_equal(tile.inverse_perm(inv).numpy(), perm)


@pytest.mark.parametrize("origin", ((-1, 0), (5, 0)))
def test_a_window_that_does_not_hold_the_tile_is_refused(origin):
    with pytest.raises(AssertionError, match="the window must contain the tile at origin"):
        tile.window_index((5, 7), origin, 3, 2)


@pytest.mark.gpu
def test_gpu_permute_planes_and_back(engine):
    """33 planes of 3 x 2 -- one more than a launch takes -- through a fixed permutation and back through its inverse."""
    ni, nj = 3, 2
    perm_h = np.array(FIXED[6], np.int32)
    planes_h = np.arange(33 * 6, dtype=np.float32).reshape(33, nj, ni)
    perm = torch.from_numpy(perm_h).cuda()
    planes = [torch.from_numpy(p).cuda() for p in planes_h]
    out = tile.permute_planes(engine, planes, perm, ni, nj)
    assert len(out) == 33
    for f in range(33):
        assert np.array_equal(out[f].cpu().numpy(), planes_h[f].reshape(-1)[perm_h].reshape(nj, ni)), f
        assert np.array_equal(tile.to_tile_order(engine, out[f], perm, ni, nj).cpu().numpy(), planes_h[f]), f
    given = [torch.full_like(p, -1.0) for p in planes]
    assert tile.permute_planes(engine, planes, perm, ni, nj, out=given)[32] is given[32]
    assert np.array_equal(given[32].cpu().numpy(), out[32].cpu().numpy())
    assert tile.to_tile_order(engine, planes[0], None, ni, nj) is planes[0]
