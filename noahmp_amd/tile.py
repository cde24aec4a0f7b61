"""Tile bookkeeping shared by the helper classes that follow a sorted store (Shortwave, WindTerrain, FlowNetwork, ForcingRegrid, History,
Regions, restart.fetch): the inverse of the sort permutation, the index plane of a window around the tile, and the gather of tile-order
planes into the store's column order.

A permutation `perm` (int32, what Engine.sort_store leaves in store.sort_perm) says: position p of the sorted order holds tile column
perm[p].  Plain functions; `engine` is a driver.Engine."""


def inverse_perm(perm):
    """int32, on perm's device: the position of every tile column in the sorted order (inv[perm[p]] = p)."""
    import torch
    inv = torch.empty(perm.numel(), dtype=torch.int32, device=perm.device)
    inv[perm.long()] = torch.arange(perm.numel(), dtype=torch.int32, device=perm.device)
    return inv


def check_window(window_shape, origin, ni, nj):
    """(i0, j0) = origin as ints, after the assertion that an (nj_w, ni_w) window holds the ni x nj tile with its cell (0, 0) there."""
    i0, j0 = (int(v) for v in origin)
    nj_w, ni_w = window_shape
    assert 0 <= i0 and i0 + ni <= ni_w and 0 <= j0 and j0 + nj <= nj_w, "the window must contain the tile at origin"
    return i0, j0


def window_index(window_shape, origin, ni, nj, pos=None, fill=-1, device=None):
    """A contiguous int32 (nj_w, ni_w) plane: tile cell (j, i), at window cell (j0 + j, i0 + i), holds pos[j*ni + i] (its own tile index
    when pos is None), every other cell `fill`.  With pos = inverse_perm(perm) it is the dst_index of a window call after a sort."""
    import torch
    i0, j0 = check_window(window_shape, origin, ni, nj)
    if pos is None:
        pos = torch.arange(ni * nj, dtype=torch.int32, device=device)
    index = torch.full(tuple(window_shape), fill, dtype=torch.int32, device=pos.device)
    index[j0:j0 + nj, i0:i0 + ni] = pos.reshape(nj, ni)
    return index.contiguous()


def sorted_perm(store, ni, nj):
    """store.sort_perm, after the checks every follow() makes."""
    perm = getattr(store, "sort_perm", None)
    assert perm is not None, "follow() is for a store that Engine.sort_store has sorted"
    assert store.ni == ni and store.nj == nj
    return perm


def permute_planes(engine, planes, perm, ni, nj, out=None):
    """New planes with out[f][p] = planes[f][perm[p]] (noahmp_hip_gather_fields, 32 planes per launch); out: the destinations, else fresh
    ones.  The gather runs on the engine's stream while torch made its operands on its own: so torch's current stream and the engine's
    stream are waited for before, and the engine's stream after."""
    import torch
    planes = list(planes)
    out = [torch.empty_like(t) for t in planes] if out is None else list(out)
    torch.cuda.current_stream().synchronize()
    engine.stream_sync()
    for i in range(0, len(planes), 32):
        engine.gather(out[i:i + 32], planes[i:i + 32], perm, ni, nj)()
    engine.stream_sync()
    return out


def to_tile_order(engine, plane, perm, ni, nj):
    """A tile-order copy of a plane in the column order of perm; the plane itself when perm is None."""
    if perm is None:
        return plane
    return permute_planes(engine, [plane], inverse_perm(perm), ni, nj)[0]
