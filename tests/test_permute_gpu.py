"""The permutation kernels of noahmp_forcing.hip (noahmp_scatter_kernel, noahmp_scatter_big_kernel<2048 / 4096 / 8192 / 16384>,
noahmp_gather_kernel) at the shapes that select each variant, against numpy indexing, bit for bit.

Every value is a bit pattern built from its level and its source column, so a misplaced element identifies itself; a few NaN (quiet,
signalling, negative) and -0.0 patterns ride along, and everything is compared as uint32.  Per shape and permutation (a random one and
a grouped one -- the stable sort of ~40 group labels, the real use: long destination runs, the same `order` values in every chunk):
tile -> sorted with fields of 1, 4 and 2 levels (the last first-level-only), sorted -> tile into the interior of a larger sentinel-
filled block (ni_mem = ni + 5, i_off = 2, j_off = 3), tile -> sorted again from that block, and the plain gather.

Found by this test: noahmp_scatter_big_kernel moved its elements in groups of 8 whatever the chunk, so the 2048- and 4096-column variants
(2 and 4 elements per thread) indexed their plan registers out of range and their sorted -> tile direction stored nothing at all
(7 x 65000 and 1153 x 769 below: every interior word still the sentinel).  The group is now min(8, elements per thread)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENT = 0xCAFEF00D
# (ni, nj) -> the chunk noahmp_hip_scatter_chunk_of must return (thresholds: 200 * chunk columns); no column count is a multiple of its chunk
SHAPES = [(333, 37, 1024),
          (7, 65000, 2048),         # rows much shorter than the 1024-thread stride: the row carry runs ~146 times per element
          (1153, 769, 4096),
          (1601, 1031, 8192),       # 1 650 631 columns
          (2051, 1601, 16384),
          (3, 70001, 1024)]         # nj > 65535: the big kernels pack the destination row into 16 bits, so the small one serves it


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _down(t):
    return t.cpu().numpy().view(np.uint32)


def _sentinel(shape):
    import torch
    return torch.full(shape, int(np.uint32(SENT).view(np.int32)), dtype=torch.int32, device="cuda")


def _fields(ni, nj):
    """three fields of 1, 4 and 2 levels: (level tag << 28) | source column; level tags 1, 2..5, 6..7"""
    col = np.arange(ni * nj, dtype=np.uint32).reshape(nj, ni)
    a = np.uint32(1 << 28) | col
    b = np.stack([np.uint32((2 + l) << 28) | col for l in range(4)], axis=1)
    c = np.stack([np.uint32((6 + l) << 28) | col for l in range(2)], axis=1)
    a.flat[5], a.flat[(ni * nj) // 2] = 0x7FC00001, 0x80000000
    b[1, 2, min(3, ni - 1)], b[nj - 1, 3, ni - 1] = 0xFFC12345, 0x80000000
    c[0, 0, 1], c[nj // 2, 1, 0] = 0x7F800001, 0xFFFFFFFF
    return [a, b, c]


def _permute(a, p):
    """column q of the result = column p[q] of a ((nj, ni) or (nj, nk, ni))"""
    if a.ndim == 2:
        return a.reshape(-1)[p].reshape(a.shape)
    nj, nk, ni = a.shape
    return np.ascontiguousarray(a.transpose(0, 2, 1).reshape(-1, nk)[p].reshape(nj, ni, nk).transpose(0, 2, 1))


def _perm(kind, n):
    r = np.random.Generator(np.random.Philox(20260 + n % 1000))
    if kind == "random":
        return r.permutation(n).astype(np.int32)
    return np.argsort(r.integers(0, 40, size=n), kind="stable").astype(np.int32)


def _eq(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d words differ, first at %s: 0x%08x instead of 0x%08x" % (what, len(bad), got.size, i, got[i], want[i]))


@pytest.mark.parametrize("kind", ["random", "grouped"])
@pytest.mark.parametrize("ni,nj,chunk", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_permutation_kernels_equal_numpy_indexing(engine, ni, nj, chunk, kind):
    import torch
    assert engine.lib.noahmp_hip_scatter_chunk_of(ni, nj) == chunk and (ni * nj) % chunk != 0
    n = ni * nj
    p = _perm(kind, n)
    src_h = _fields(ni, nj)
    want = [_permute(a, p) for a in src_h]                    # sorted position q holds tile column p[q]
    want_first = want[2].copy()
    want_first[:, 1, :] = SENT                                 # first-level-only: level 2 of the destination untouched
    perm, src = _up(p), [_up(a) for a in src_h]

    # tile -> sorted
    dst = [_sentinel(t.shape) for t in src]
    torch.cuda.synchronize()
    sc = engine.scatter(dst, src, perm, ni, nj, first_level_only=(2,))
    sc()
    engine.stream_sync()
    for f, w in enumerate((want[0], want[1], want_first)):
        _eq(_down(dst[f]), w, "tile -> sorted, field %d" % f)

    # sorted -> tile, into the interior of a larger block
    i_off, j_off, ni_mem, nj_mem = 2, 3, ni + 5, nj + 5
    block = [_sentinel((nj_mem,) + tuple(t.shape[1:-1]) + (ni_mem,)) for t in src]
    torch.cuda.synchronize()
    sc.exchange(dst, block, True, ni_mem=ni_mem, i_off=i_off, j_off=j_off, first_level_only=(2,))
    engine.stream_sync()
    back_first = src_h[2].copy()
    back_first[:, 1, :] = SENT
    for f, w in enumerate((src_h[0], src_h[1], back_first)):
        got = _down(block[f])
        _eq(got[j_off:j_off + nj, ..., i_off:i_off + ni], w, "sorted -> tile, interior of field %d" % f)
        ring = np.ones(got.shape, dtype=bool)
        ring[j_off:j_off + nj, ..., i_off:i_off + ni] = False
        assert (got[ring] == SENT).all(), "sorted -> tile wrote %d ring cells of field %d" % ((got[ring] != SENT).sum(), f)

    # tile -> sorted from the same offset block
    dst2 = [_sentinel(t.shape) for t in src]
    torch.cuda.synchronize()
    sc.exchange(dst2, block, False, ni_mem=ni_mem, i_off=i_off, j_off=j_off, first_level_only=(2,))
    engine.stream_sync()
    for f, w in enumerate((want[0], want[1], want_first)):
        _eq(_down(dst2[f]), w, "offset block -> sorted, field %d" % f)

    # the plain gather with the same permutation (every level travels)
    dst3 = [_sentinel(t.shape) for t in src]
    torch.cuda.synchronize()
    engine.gather(dst3, src, perm, ni, nj)()
    engine.stream_sync()
    for f in range(3):
        _eq(_down(dst3[f]), want[f], "gather, field %d" % f)


@pytest.mark.parametrize("ni,nj", [(333, 37), (1153, 769)])
def test_output_fields_masks_water_points_of_masked_fields_only(engine, ni, nj):
    """noahmp_hip_output_fields: dst column q <- src column perm[q]; -1.E33 where IVGTYP (in SOURCE order) is water, for the fields whose
    mask bit is set, and the gathered value everywhere else"""
    import torch
    n, iswater, mask = ni * nj, 16, 0b101
    r = np.random.Generator(np.random.Philox(777))
    inv = r.permutation(n).astype(np.int32)
    ivg = np.where(r.random(n) < 0.2, iswater, r.integers(1, 16, size=n)).astype(np.int32).reshape(nj, ni)
    src_h = _fields(ni, nj)
    water = (ivg.reshape(-1) == iswater)[inv].reshape(nj, ni)           # tile column q shows source column inv[q]
    assert 0.15 * n < water.sum() < 0.25 * n
    missing = np.float32(-1.0e33).view(np.uint32)
    want = [_permute(a, inv) for a in src_h]
    for f in (0, 2):
        want[f][np.broadcast_to(water[:, None, :] if want[f].ndim == 3 else water, want[f].shape)] = missing
    src, perm, veg = [_up(a) for a in src_h], _up(inv), _up(ivg)
    dst = [_sentinel(t.shape) for t in src]
    torch.cuda.synchronize()
    args = ((C.c_void_p * 3)(*[t.data_ptr() for t in dst]), (C.c_void_p * 3)(*[t.data_ptr() for t in src]), (C.c_int * 3)(1, 4, 2), perm.data_ptr())
    # masking without IVGTYP: refused, nothing launched
    assert engine.lib.noahmp_hip_output_fields(3, *args, None, iswater, mask, ni, nj, None) == -105
    engine.stream_sync()
    for f in range(3):
        assert (_down(dst[f]) == SENT).all()
    assert engine.lib.noahmp_hip_output_fields(3, *args, veg.data_ptr(), iswater, mask, ni, nj, None) == 0
    engine.stream_sync()
    for f in range(3):
        _eq(_down(dst[f]), want[f], "output_fields, field %d" % f)
    assert (want[1] != missing).all() and (want[0] == missing).sum() == water.sum()
