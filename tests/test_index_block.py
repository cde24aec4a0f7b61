"""Every entry point that takes the caller's WRF index block (ids..kte), at index blocks shaped like WRF's: kme > 2, kms = 0 or below,
halos, shifted origins, kts > 1.  The rest of the suite drives the library with kms = 1, kme = 2, kts = 1, where k1 = kp_lo = 0,
kp_hi = 1 and nka = 2: a kernel that used one of them for another would pass it.

The mechanism is EMBEDDING.  embed() places the tile of a compact store (memory == tile, kms:kme = 1:2) inside a larger memory block.
Everything around the tile -- halo cells, the atmospheric levels the call does not read -- is filler that is valid but different: the
columns of a store made with another seed at another hour, the level's own values times 1 + 0.03 * (slot + 1).  A wrong read then gives
a plausible wrong answer (no NaN, no table index out of range, no fault).  Every test asserts two things bit for bit (uint32 views, so
NaN equals the same NaN; no tolerance anywhere): (a) the words the call writes in the tile are those of the ORACLE ON THE COMPACT STORE,
(b) every other word -- outside the tile, atmospheric levels the contract does not write -- has the bits it had before the call.

One block has no compact twin: E7 (kts = 2 with another pressure at level 1 than at level kts, the only block that tells kp_lo from
k1).  Its reference is the oracle on the same block, which C2 holds against the compiled reference there.

C1-C5 need no GPU (C5: the index-block refusals of include/noahmp_hip.h, which are made before the device is initialised); G1-G7 are
the same claims through the C-ABI on the device.  No bad block is ever passed in a gpu test."""
import ctypes as C
import functools

import numpy as np
import pytest

from noahmp_amd import abi, synth
from noahmp_amd.abi import FIELD_INFO
from noahmp_amd.state import ColumnStore, ModelConfig

F = np.float32
ATM = tuple(n for n in abi.ARRAY_FIELDS if FIELD_INFO[n][1] == "atm")        # dz8w t3d qv3d u_phy v_phy p8w3d
NI, NJ = 35, 5                                                              # 175 columns: two full waves and a ragged one
YR, JULIAN = 2000, 180.0

#            halo l, r, b, t        kms:kme          kts      origin (its, jts)
CASES = {
    "E1": dict(halo=(0, 0, 0, 0), kms=1, kme=5, kts=1, origin=(1, 1)),
    "E2": dict(halo=(0, 0, 0, 0), kms=0, kme=3, kts=1, origin=(1, 1)),
    "E3": dict(halo=(0, 0, 0, 0), kms=-2, kme=4, kts=1, origin=(1, 1)),
    "E4": dict(halo=(3, 1, 2, 1), kms=1, kme=2, kts=1, origin=(17, -4)),
    "E5": dict(halo=(1, 4, 0, 3), kms=0, kme=6, kts=1, origin=(-9, 30)),
    "E6": dict(halo=(2, 2, 1, 1), kms=1, kme=4, kts=2, origin=(1, 1)),          # kts = 2: the pressure slots are not k1, k1 + 1
}
ALL = sorted(CASES)
# In E1-E6 level 1 of P8W3D holds the words of level kts (PSFC = P8W3D(1) is read beside P8W3D(kts), drv:463-464, and the compact store
# has one plane for both), so E6 tells kp_hi from k1 + 1 but NOT kp_lo from k1.  E7 is E6 with another pressure at level 1: it has no
# compact twin, its reference is the compiled reference and the oracle ON THE SAME BLOCK.
E7 = dict(CASES["E6"], psfc_scale=1.012)
BLOCKS = dict(CASES, E7=E7)


# ---------------------------------------------------------------------------------------------------------------- stores and embedding
@functools.lru_cache(maxsize=None)
def _tables():
    from noahmp_amd.tables import load_tables
    return load_tables("usgs")


def _forcing(s, hour):
    """diurnal_forcing, then a pressure that differs between columns and between its levels 1 and 2 (the step reads both)."""
    synth.diurnal_forcing(s, hour, t_offset=s.t_offset)
    p1 = (F(95000.0) - F(40.0) * s.t_offset).astype(F)
    s.a["p8w3d"][:, 0, :] = p1
    s.a["p8w3d"][:, 1, :] = (p1 * F(0.985)).astype(F)
    s.a["u_phy"][:, 0, :] = (F(3.0) + F(0.05) * s.t_offset).astype(F)


def compact_store(ni=NI, nj=NJ, seed=4, hour=13, cfg=None, groundwater=False):
    """The tile: synth.mixed_small plus two open-water cells and one sea-ice cell, forcing of `hour`, first-step guesses."""
    s = synth.mixed_small(_tables()[1], ni=ni, nj=nj, seed=seed, cfg=cfg)
    s.a["xland"][nj // 4, ni // 5] = 2.0
    s.a["xland"][nj - 1, ni - 2] = 2.0
    s.a["xice"][nj // 2, ni // 2] = 1.0
    if groundwater:
        synth.groundwater_fields(s, _tables()[1], seed=seed + 100, stress=0.02)
    _forcing(s, hour)
    synth.first_step_fixups(s)
    return s


_FILLERS = {}


def _filler(ni, nj, cfg, groundwater):
    """The store whose columns surround the tile (made once per shape; embed() copies out of it and never writes it)."""
    key = (ni, nj, repr(cfg), groundwater)
    if key not in _FILLERS:
        s = synth.mixed_small(_tables()[1], ni=ni, nj=nj, seed=11, cfg=cfg)   # another seed ...
        if groundwater:
            synth.groundwater_fields(s, _tables()[1], seed=211, stress=0.02)
        _forcing(s, 16)                                                        # ... and another hour
        synth.first_step_fixups(s)
        _FILLERS[key] = s
    return _FILLERS[key]


def tile_slices(idx):
    return (slice(idx["jts"] - idx["jms"], idx["jte"] - idx["jms"] + 1), slice(idx["its"] - idx["ims"], idx["ite"] - idx["ims"] + 1))


def embed_plane(compact, filler, idx):
    """A 2-D plane shaped like the memory block: the filler's cells around the compact plane."""
    out = np.array(filler, copy=True)
    jsl, isl = tile_slices(idx)
    out[jsl, isl] = compact
    return out


def embed(compact, halo=(0, 0, 0, 0), kms=1, kme=2, kts=1, origin=(1, 1), domain=None, psfc_scale=None):
    """The tile of `compact` (memory == tile, kms:kme = 1:2) inside a memory block with `halo` = (left, right, bottom, top) cells around
    it and atmospheric levels kms:kme, its first cell at Fortran index `origin`.  domain: ids, ide, jds, jde (default: the memory block).
    psfc_scale (kts >= 2 only): level 1 of P8W3D holds the plane of level kts times this factor instead of its words."""
    left, right, bottom, top = halo
    ni, nj = compact.ni, compact.nj
    nim, njm, nka = ni + left + right, nj + bottom + top, kme - kms + 1
    its, jts = origin
    idx = dict(ims=its - left, ime=its + ni - 1 + right, jms=jts - bottom, jme=jts + nj - 1 + top, kms=kms, kme=kme,
               its=its, ite=its + ni - 1, jts=jts, jte=jts + nj - 1, kts=kts, kte=kts, kds=kms, kde=kme)
    ids, ide, jds, jde = domain or (idx["ims"], idx["ime"], idx["jms"], idx["jme"])
    idx.update(ids=ids, ide=ide, jds=jds, jde=jde)
    fill = _filler(nim, njm, compact.cfg, "fdepth" in compact.a)
    out = ColumnStore(nim, njm, compact.cfg)
    jsl, isl = tile_slices(idx)
    for k, v in fill.a.items():
        if k == "dzs":
            continue
        if k not in ATM:
            out.a[k] = np.array(v, copy=True)
            out.a[k][jsl, ..., isl] = compact.a[k]
            continue
        lev1 = embed_plane(compact.a[k][:, 0, :], v[:, 0, :], idx)
        arr = np.empty((njm, nka, nim), F)
        for slot in range(nka):
            arr[:, slot, :] = lev1 * F(1.0 + 0.03 * (slot + 1))
        arr[:, 1 - kms, :] = lev1
        if k == "p8w3d":                                 # SFCPRS = (P8W3D(kts+1) + P8W3D(kts)) * 0.5, drv:463
            arr[:, kts - kms, :] = lev1
            arr[:, kts + 1 - kms, :] = embed_plane(compact.a[k][:, 1, :], v[:, 1, :], idx)
            if psfc_scale is not None:
                assert kts >= 2
                arr[:, 1 - kms, :] = lev1 * F(psfc_scale)
        out.a[k] = arr
    out.set_index(**idx)
    return out


def place(block, compact, atm_levels=None):
    """`block` with the tile's words replaced by those of `compact`: every non-atmospheric array, and of the atmospheric array n the
    levels atm_levels[n] (Fortran level numbers; the step writes none)."""
    idx = block.index()
    jsl, isl = tile_slices(idx)
    for k, v in compact.a.items():
        if k == "dzs":
            continue
        if k in ATM:
            for lev in (atm_levels or {}).get(k, ()):
                block.a[k][jsl, lev - idx["kms"], isl] = v[:, lev - 1, :]
        else:
            block.a[k][jsl, ..., isl] = v
    return block


def words(x):
    return np.ascontiguousarray(x).view(np.uint32)


def assert_bits(got, want, what, atm_levels=None, planes=()):
    """(a) the tile's written words equal `want`'s, (b) every other word does; `want` = place(the block before the call, oracle result).
    planes: further (name, got, want) 2-D planes shaped like the memory block."""
    idx = want.index()
    jsl, isl = tile_slices(idx)
    bad_in, bad_out = [], []
    items = [(k, got.a[k], want.a[k]) for k in want.a if k != "dzs"] + list(planes)
    for k, x, y in items:
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape)
        d = words(x) != words(y)
        m = np.zeros(d.shape, bool)
        if k in ATM:
            for lev in (atm_levels or {}).get(k, ()):
                m[jsl, lev - idx["kms"], isl] = True
        else:
            m[jsl, ..., isl] = True
        if (d & m).any():
            bad_in.append("%s: %d words, first at %s" % (k, int((d & m).sum()), np.argwhere(d & m)[0].tolist()))
        if (d & ~m).any():
            bad_out.append("%s: %d words, first at %s" % (k, int((d & ~m).sum()), np.argwhere(d & ~m)[0].tolist()))
    assert np.array_equal(got.a["dzs"], want.a["dzs"])
    assert not bad_in, "%s: (a) words of the tile differ from the oracle on the compact store\n  %s" % (what, "\n  ".join(bad_in))
    assert not bad_out, "%s: (b) words the call must not write have changed\n  %s" % (what, "\n  ".join(bad_out))


def differing_columns(got, want):
    """Per tile column of `got` (a block): does any word of a non-input array differ from the compact store `want`?"""
    jsl, isl = tile_slices(got.index())
    diff = np.zeros((want.nj, want.ni), bool)
    for k, v in want.a.items():
        if k == "dzs" or FIELD_INFO.get(k, (0, 0, "in"))[2] == "in":
            continue
        d = words(got.a[k][jsl, ..., isl]) != words(v)
        diff |= d.any(axis=1) if d.ndim == 3 else d
    return diff


@pytest.fixture(scope="module")
def compact():
    return compact_store()


@pytest.fixture(scope="module")
def stepped(port, compact):
    """The oracle's first step on the compact store: the reference of every step test (computed once, never changed)."""
    s = compact.copy()
    st = port.noahmplsm(s, 1, YR, JULIAN)
    assert st.code == 0 and st.n_land + st.n_glacier + st.n_skipped == NI * NJ
    assert st.n_land >= 128 and st.n_glacier >= 4 and st.n_skipped == 3, (st.n_land, st.n_glacier, st.n_skipped)
    return s


@pytest.fixture(scope="module")
def emul():
    from host_emul.emullib import EmulLib
    e = EmulLib()
    e.set_tables(_tables()[0])
    return e


def test_embed_layout(compact):
    """The helper itself: extents, the slots of levels 1 / kts / kts+1, and filler that differs from the tile's values everywhere."""
    e = embed(compact, **CASES["E6"])
    idx = e.index()
    assert (idx["ims"], idx["ime"], idx["jms"], idx["jme"]) == (-1, 37, 0, 6) and e.a["t3d"].shape == (7, 4, 39)
    jsl, isl = tile_slices(idx)
    assert np.array_equal(e.a["t3d"][jsl, 0, isl], compact.a["t3d"][:, 0, :])
    assert np.array_equal(e.a["p8w3d"][jsl, 1, isl], compact.a["p8w3d"][:, 0, :])
    assert np.array_equal(e.a["p8w3d"][jsl, 2, isl], compact.a["p8w3d"][:, 1, :])
    assert (e.a["p8w3d"][jsl, 2, isl] != e.a["p8w3d"][jsl, 1, isl]).all()
    for k in ATM:
        lev1 = e.a[k][:, 0, :]
        for slot in range(1, 4):
            if k == "p8w3d" and slot in (1, 2):
                continue
            assert (e.a[k][:, slot, :] != lev1).all() and np.isfinite(e.a[k][:, slot, :]).all(), (k, slot)
    e5 = embed(compact, **CASES["E5"])
    assert (e5.index()["its"], e5.index()["jts"], e5.index()["ims"], e5.index()["jme"]) == (-9, 30, -10, 37)
    assert e5.a["tsk"].shape == (8, 40) and e5.a["qv3d"].shape == (8, 7, 40)


# ---------------------------------------------------------------------------------------------------------------- C1-C4: CPU
@pytest.mark.parametrize("case", ALL)
def test_c1_oracle_is_embedding_invariant(port, compact, stepped, case):
    e = embed(compact, **CASES[case])
    before = e.copy()
    st = port.noahmplsm(e, 1, YR, JULIAN)
    assert st.code == 0
    assert_bits(e, place(before, stepped), "oracle step " + case)


def test_c1_oracle_kts2_block_with_its_own_level_1_pressure(port, compact, stepped):
    """E7: the oracle writes the tile only, and PSFC from level 1 matters (the tile is no longer the compact result), so a read of
    P8W3D(kts) at level 1 -- or of PSFC at level kts -- changes bits."""
    e = embed(compact, **E7)
    before = e.copy()
    assert port.noahmplsm(e, 1, YR, JULIAN).code == 0
    jsl, isl = tile_slices(e.index())
    for k in e.a:
        halo = np.ones(e.a[k].shape, bool)
        if k != "dzs" and k not in ATM:
            halo[jsl, ..., isl] = False
        assert np.array_equal(words(e.a[k])[halo], words(before.a[k])[halo]), k
    e6 = embed(compact, **CASES["E6"])
    port.noahmplsm(e6, 1, YR, JULIAN)
    changed = differing_columns(e, stepped)
    assert changed.mean() > 0.5 and not differing_columns(e6, stepped).any(), changed.mean()


def _init_inputs(s, marker, where=None):
    """What a caller hands to NOAHMP_INIT: every array it writes except the ones it also reads holds a marker (`where`: a mask over
    (j, i), default everywhere)."""
    from test_init import INIT_FIELDS
    for k in INIT_FIELDS:
        if k not in ("snow", "snowh", "tslb", "smois", "sh2o"):
            v = s.a[k]
            m = np.ones(v.shape, bool) if where is None else (where[:, None, :] if v.ndim == 3 else where) & np.ones(v.shape, bool)
            v[m] = marker if v.dtype.kind == "f" else int(-marker) % 97
    return s


def _run_init(lib_call, store, bump):
    a = store.step_args(1, YR, 1.0)
    a.ide += bump
    a.jde += bump
    st = abi.Status()
    rc = lib_call(a, st)
    assert rc == 0 and st.code == 0, (rc, st.code)


def _init_pairs(compact, cases=("E4", "E5")):
    """(name, compact store, embedded block, ide / jde bump of the compact call, of the embedded call).  `interior`: the domain ends
    beyond the tile, so the whole tile is initialised; `edge`: ite = ide and jte = jde, where NOAHMP_INIT stops at ide-1 / jde-1."""
    c = _init_inputs(compact.copy(), -777.0)
    out = []
    for case in cases:
        for name in ("interior", "edge"):
            g = CASES[case]
            its, jts = g["origin"]
            dom = (its - 20, its + NI - 1 + (9 if name == "interior" else 0), jts - 20, jts + NJ - 1 + (9 if name == "interior" else 0))
            e = embed(c, domain=dom, **g)
            halo = np.ones((e.nj, e.ni), bool)             # the halo holds another marker: a column initialised there shows
            halo[tile_slices(e.index())] = False
            _init_inputs(e, -555.0, halo)
            out.append(("%s-%s" % (case, name), c, e, 1 if name == "interior" else 0, 0))
    return out


def _check_init(call, port, compact, cases=("E4", "E5")):
    for name, c, e, bump_c, bump_e in _init_pairs(compact, cases):
        want_c = c.copy()
        _run_init(lambda a, st: port.lib.nmp_oracle_init(C.byref(a), c.cfg.iswater, 1, C.byref(st)), want_c, bump_c)
        if name.endswith("edge"):                          # the clamp bit: the last row and column keep their markers
            assert (want_c.a["tvxy"][-1, :] == -777.0).all() and (want_c.a["tvxy"][:, -1] == -777.0).all()
            assert (want_c.a["tvxy"][:-1, :-1] != -777.0).mean() > 0.9
        before = e.copy()
        _run_init(lambda a, st: call(a, e.cfg.iswater, st), e, bump_e)
        assert_bits(e, place(before, want_c), "noahmp_init " + name)


def _gw_compact():
    return compact_store(seed=4, cfg=ModelConfig(iopt_run=5), groundwater=True)


def _assert_block_equal(a, b, what, names=None):
    """Two blocks of the same shape hold the same words (the inter-column calls: the reference is the oracle ON THE SAME BLOCK)."""
    bad = []
    for k in (names or a.a):
        if not np.array_equal(words(a.a[k]), words(b.a[k])):
            d = words(a.a[k]) != words(b.a[k])
            bad.append("%s: %d words, first at %s" % (k, int(d.sum()), np.argwhere(d)[0].tolist()))
    assert not bad, "%s\n  %s" % (what, "\n  ".join(bad))


@pytest.mark.parametrize("case", ["E2", "E5", "E6", "E7"])
def test_c2_oracle_equals_compiled_reference(port, reflib, compact, case):
    """The oracle against the unmodified reference at blocks other than kms:kme = 1:2: its k1 (E2, E5), kts + 1 (E6) and, in E7 only,
    which of level 1 and level kts of the pressure goes where."""
    reflib.set_tables(_tables()[0])
    e = embed(compact, **BLOCKS[case])
    a, b = e.copy(), e.copy()
    reflib.noahmplsm(a, 1, YR, JULIAN)
    assert port.noahmplsm(b, 1, YR, JULIAN).code == 0
    _assert_block_equal(a, b, "noahmplsm " + case)
    assert not np.array_equal(words(a.a["tslb"]), words(e.a["tslb"]))
    # cold start (the reference's wrapper passes ide + 1 / jde + 1, as hdrv:291 does)
    if case == "E7":                      # the rest does not read the pressure: E6 has run it
        return
    its, jts = CASES[case]["origin"]
    c = _init_inputs(compact.copy(), -777.0)
    e = embed(c, domain=(its - 20, its + NI + 8, jts - 20, jts + NJ - 2), **CASES[case])       # jte = jde + 1: the clamp bites in j
    a, b = e.copy(), e.copy()
    reflib.noahmp_init(a)
    _run_init(lambda s, st: port.lib.nmp_oracle_init(C.byref(s), e.cfg.iswater, 1, C.byref(st)), b, 1)
    _assert_block_equal(a, b, "noahmp_init " + case)
    jsl, isl = tile_slices(e.index())
    assert (b.a["tvxy"][jsl, isl][-1] == -777.0).all() and (b.a["tvxy"][jsl, isl][:-1] != -777.0).mean() > 0.9
    # groundwater
    reflib.set_tables(_tables()[0])
    e = embed(_gw_compact(), **CASES[case])
    a, b = e.copy(), e.copy()
    reflib.wtable_mmf(a)
    port.wtable_mmf(b)
    _assert_block_equal(a, b, "wtable_mmf " + case)
    assert not np.array_equal(words(a.a["zwtxy"]), words(e.a["zwtxy"]))


@pytest.mark.parametrize("case", ALL)
def test_c3_device_source_step(emul, compact, stepped, case):
    e = embed(compact, **CASES[case])
    before = e.copy()
    st = emul.noahmplsm(e, 1, YR, JULIAN)
    assert st.code == 0 and st.n_skipped == 3
    assert_bits(e, place(before, stepped), "device source, step " + case)


def test_c3_device_source_step_kts2_block(emul, port, compact):
    """E7 against the oracle on the same block (which test_c2 holds against the compiled reference): kp_lo is not k1."""
    e = embed(compact, **E7)
    a, b = e.copy(), e.copy()
    assert port.noahmplsm(a, 1, YR, JULIAN).code == 0 and emul.noahmplsm(b, 1, YR, JULIAN).code == 0
    _assert_block_equal(b, a, "device source, step E7")


# ---- forcing: records, longitude and rain rate shaped like the memory block
WHEN = (171, 14, 20, 30)
IDTS, IDTS2 = 1800, 10800
LEV1 = {k: (1,) for k in ("t3d", "qv3d", "u_phy", "v_phy", "p8w3d")}
LEV12 = {k: (1, 2) for k in ATM}


def _records(ni, nj, seed):
    r = np.random.default_rng(seed)
    rng = dict(t=(250, 310), q=(1e-4, 2e-2), u=(-10, 10), v=(-10, 10), p=(6e4, 1.02e5), lw=(150, 450), sw=(0, 1000),
               pcp=(0, 2e-3), fpar=(0, 1), lai=(0, 6))
    recs = [{k: r.uniform(lo, hi, size=(nj, ni)).astype(F) for k, (lo, hi) in rng.items()} for _ in range(2)]
    lon = r.uniform(-180.0, 180.0, size=(nj, ni)).astype(F)
    rain = r.uniform(0.0, 2e-3, size=(nj, ni)).astype(F)
    return recs[0], recs[1], lon, rain


@pytest.fixture(scope="module")
def forcing_ref(port, compact):
    """The oracle's interpolation and preparation on the compact store (computed once)."""
    ra, rb, lon, rain0 = _records(NI, NJ, 31)
    s1 = compact.copy()
    rain = np.array(rain0, copy=True)
    port.forcing_interpolate(s1, ra, rb, IDTS, IDTS2, rain)
    s2 = s1.copy()
    jul = port.forcing_prep(s2, lon, rain, *WHEN, scale_vegfra=True, first_step=True)
    assert not np.array_equal(s2.a["t3d"][:, 1, :], compact.a["t3d"][:, 1, :])
    return dict(ra=ra, rb=rb, lon=lon, rain0=rain0, interp=s1, rain=rain, prep=s2, julian=jul)


def _forcing_block(compact, ref, case):
    e = embed(compact, **CASES[case])
    idx = e.index()
    fa, fb, flon, frain = _records(e.ni, e.nj, 47)
    ra = {k: embed_plane(ref["ra"][k], fa[k], idx) for k in fa}
    rb = {k: embed_plane(ref["rb"][k], fb[k], idx) for k in fb}
    return e, ra, rb, embed_plane(ref["lon"], flon, idx), embed_plane(ref["rain0"], frain, idx), frain


def _check_forcing(interpolate, prep, compact, ref, case, who):
    """interpolate(block, ra, rb, rain) and prep(block, lon, rain) of one implementation, on the embedded block."""
    e, ra, rb, lon, rain, frain = _forcing_block(compact, ref, case)
    idx = e.index()
    before = e.copy()
    interpolate(e, ra, rb, rain)
    assert_bits(e, place(before, ref["interp"], LEV1), "%s forcing_interpolate %s" % (who, case), LEV1,
                planes=[("rain_rate", rain, embed_plane(ref["rain"], frain, idx))])
    before = e.copy()
    prep(e, lon, rain)
    assert_bits(e, place(before, ref["prep"], LEV12), "%s forcing_prep %s" % (who, case), LEV12)


@pytest.mark.parametrize("case", ALL)
def test_c1_oracle_forcing_is_embedding_invariant(port, compact, forcing_ref, case):
    _check_forcing(lambda s, ra, rb, rain: port.forcing_interpolate(s, ra, rb, IDTS, IDTS2, rain),
                   lambda s, lon, rain: port.forcing_prep(s, lon, rain, *WHEN, scale_vegfra=True, first_step=True),
                   compact, forcing_ref, case, "oracle")


@pytest.mark.parametrize("case", ALL)
def test_c3_device_source_forcing(emul, compact, forcing_ref, case):
    lib = abi.load_library()                      # host-only entry of the product library (no GPU call)
    iday, h, m, sec = WHEN
    sd, cd = C.c_float(0), C.c_float(0)
    lib.noahmp_hip_declination(iday, h, C.byref(sd), C.byref(cd))
    hour = F(F(F(h) + F(m) / F(60.0)) + F(sec) / F(3600.0))
    _check_forcing(lambda s, ra, rb, rain: emul.forcing_interpolate(s, ra, rb, IDTS, IDTS2, rain),
                   lambda s, lon, rain: emul.forcing_prep(s, lon, rain, float(hour), sd.value, cd.value, scale_vegfra=True, first_step=True),
                   compact, forcing_ref, case, "device source,")


def test_c3_device_source_init(emul, port, compact):
    _check_init(lambda a, iswater, st: emul.lib.emul_init(C.byref(a), iswater, 1, C.byref(st)), port, compact, ALL)


@pytest.mark.parametrize("case", ALL)
def test_c3_device_source_groundwater(emul, port, case):
    e = embed(_gw_compact(), **CASES[case])
    a, b = e.copy(), e.copy()
    sa, sb = port.wtable_mmf(a), emul.wtable_mmf(b)
    assert sa.n_land == sb.n_land and sa.n_land > 100
    _assert_block_equal(a, b, "wtable_mmf " + case)
    assert not np.array_equal(words(a.a["zwtxy"]), words(e.a["zwtxy"])) and (a.a["qslat"] != 0).any()
    a, b = e.copy(), e.copy()
    port.groundwater_init(a)
    emul.groundwater_init(b)
    _assert_block_equal(a, b, "groundwater_init " + case)
    assert not np.array_equal(words(a.a["smoiseq"]), words(e.a["smoiseq"]))


def test_c4_the_test_can_fail(port, compact, stepped):
    """A condition on the filler, not a measurement: with kms:kme declared one higher than the truth the oracle reads level 1 from the
    filler one slot down, and at least 90 % of the columns that are advanced must then differ from the compact result."""
    g = dict(CASES["E5"])
    e = embed(compact, **g)
    e.set_index(kms=g["kms"] + 1, kme=g["kme"] + 1, kds=g["kms"] + 1, kde=g["kme"] + 1)
    port.noahmplsm(e, 1, YR, JULIAN)
    advanced = ~((compact.a["xland"] - F(1.5) >= 0) | (compact.a["xice"] >= F(compact.cfg.xice_thres)))
    diff = differing_columns(e, stepped) & advanced
    share = diff.sum() / advanced.sum()
    assert share >= 0.9, "only %d of %d advanced columns (%.1f %%) differ when level 1 is read from the filler" % (
        diff.sum(), advanced.sum(), 100.0 * share)
    right = embed(compact, **g)
    port.noahmplsm(right, 1, YR, JULIAN)
    assert not differing_columns(right, stepped).any()


# ---------------------------------------------------------------------------------------------------------------- C5: refusals
POISON = 7.0
BASE = dict(ids=1, ide=100, jds=1, jde=100, kds=1, kde=2, ims=1, ime=6, jms=1, jme=4, kms=1, kme=2, its=2, ite=5, jts=2, jte=3, kts=1, kte=1)
# (overrides of the index block, the bound the text must name)
RULES_ALL = [(dict(ime=-1), "ime"), (dict(jme=-1), "jme"), (dict(kms=1, kme=0), "kme"), (dict(kms=2, kme=3), "kms"),
             (dict(kms=-1, kme=0), "kme"), (dict(its=0), "its"), (dict(ite=7), "ite"), (dict(jts=0), "jts"), (dict(jte=5), "jte"),
             (dict(its=-3, ite=0, ims=-1, ime=6), "its")]
RULES_STEP = [(dict(kme=1), "kts"), (dict(kts=2), "kts"), (dict(kts=0), "kts"), (dict(kms=0, kme=3, kts=3), "kts"), (dict(ite=7), "ite")]
RULES_PREP = [(dict(kms=0, kme=1), "kme"), (dict(kms=2, kme=3), "kms"), (dict(kms=-3, kme=1), "kme")]


class _Poisoned:
    """Host arrays full of a poison value behind a step block; nothing a refused call is given may lose it."""

    def __init__(self):
        self.s = ColumnStore(6, 4, fill=POISON)
        self.s.a["dzs"][...] = POISON
        for k in ATM:
            self.s.a[k] = np.full((4, 8, 6), POISON, F)
        self.t = ColumnStore(6, 4, fill=POISON)
        self.t.a["dzs"][...] = POISON
        for k in ATM:
            self.t.a[k] = np.full((4, 8, 6), POISON, F)
        self.planes = {k: np.full((4, 6), POISON, F) for k in ("lon", "rain") + abi.FORCING_RECORD_FIELDS}
        self.perm = np.full(24, 7, np.int32)
        self.keys = np.full(24, 7, np.uint32)
        self.counts = (C.c_int64 * 3)(7, 7, 7)
        self.changed = C.c_int64(7)
        self.jul = C.c_float(POISON)
        self.st = abi.Status()

    def args(self, store, **over):
        a = store.step_args(1, YR, 1.0)
        for k, v in dict(BASE, **over).items():
            setattr(a, k, v)
        return a

    def record(self):
        r = abi.ForcingRecord()
        for n in abi.FORCING_RECORD_FIELDS:
            setattr(r, n, self.planes[n].ctypes.data)
        return r

    def untouched(self):
        for s in (self.s, self.t):
            for k, v in s.a.items():
                assert (v == (POISON if v.dtype.kind == "f" else 7)).all(), k
        for k, v in self.planes.items():
            assert (v == POISON).all(), k
        assert (self.perm == 7).all() and (self.keys == 7).all() and list(self.counts) == [7, 7, 7] and self.jul.value == POISON
        assert self.changed.value == 7


def _entries(lib, p):
    """name -> (call(a) -> rc, extra rules of the entry point)"""
    ra, rb = p.record(), p.record()
    lon, rain = p.planes["lon"].ctypes.data, p.planes["rain"].ctypes.data
    D = abi.MEM_DEVICE
    return {
        "noahmp_hip_step": (lambda a: lib.noahmp_hip_step(C.byref(a), abi.MEM_HOST, None, C.byref(p.st)), RULES_STEP),
        "noahmp_hip_step_async": (lambda a: lib.noahmp_hip_step_async(C.byref(a), None), RULES_STEP),
        "noahmp_hip_init": (lambda a: lib.noahmp_hip_init(C.byref(a), 16, 1, abi.MEM_HOST, None, C.byref(p.st)), []),
        "noahmp_hip_forcing_prep": (lambda a: lib.noahmp_hip_forcing_prep(C.byref(a), lon, rain, 171, 12, 0, 0, 30.0, 3, C.byref(p.jul), D, None,
                                                                         C.byref(p.st)), RULES_PREP),
        "noahmp_hip_forcing_interpolate": (lambda a: lib.noahmp_hip_forcing_interpolate(C.byref(a), C.byref(ra), C.byref(rb), IDTS, IDTS2, rain, D,
                                                                                       None, C.byref(p.st)), []),
        "noahmp_hip_forcing_interpolate_prep": (lambda a: lib.noahmp_hip_forcing_interpolate_prep(
            C.byref(a), C.byref(ra), C.byref(rb), IDTS, IDTS2, rain, lon, 171, 12, 0, 0, 30.0, 3, C.byref(p.jul), D, None, C.byref(p.st)), RULES_PREP),
        "noahmp_hip_sort_columns": (lambda a: lib.noahmp_hip_sort_columns(C.byref(a), abi.SORT_VEG | abi.SORT_TAIR, 1000, p.perm.ctypes.data,
                                                                         p.keys.ctypes.data, p.counts, None), []),
        "noahmp_hip_sort_staleness": (lambda a: lib.noahmp_hip_sort_staleness(C.byref(a), abi.SORT_VEG | abi.SORT_TAIR, p.keys.ctypes.data,
                                                                             C.byref(p.changed), None), []),
        "noahmp_hip_sort_staleness_async": (lambda a: lib.noahmp_hip_sort_staleness_async(C.byref(a), abi.SORT_VEG | abi.SORT_TAIR,
                                                                                         p.keys.ctypes.data, None), []),
        "noahmp_hip_permute_step_arrays (src)": (lambda a: lib.noahmp_hip_permute_step_arrays(C.byref(a), C.byref(p.args(p.t)), p.perm.ctypes.data,
                                                                                             None), []),
        "noahmp_hip_permute_step_arrays (dst)": (lambda a: lib.noahmp_hip_permute_step_arrays(C.byref(p.args(p.t)), C.byref(a), p.perm.ctypes.data,
                                                                                             None), []),
    }


ENTRY_NAMES = ["noahmp_hip_step", "noahmp_hip_step_async", "noahmp_hip_init", "noahmp_hip_forcing_prep", "noahmp_hip_forcing_interpolate",
               "noahmp_hip_forcing_interpolate_prep", "noahmp_hip_sort_columns", "noahmp_hip_sort_staleness", "noahmp_hip_sort_staleness_async",
               "noahmp_hip_permute_step_arrays (src)",
               "noahmp_hip_permute_step_arrays (dst)"]


@pytest.mark.parametrize("entry", ENTRY_NAMES)
def test_c5_refusals_write_nothing(entry):
    """Every rule of the index-block text of include/noahmp_hip.h, for every entry point that takes a step block: -103, the text names
    the entry point and the bound, and nothing the call was given is written.  The check precedes the device initialisation, so this
    runs where there is no device (and where there is one, the arrays are host memory no kernel could reach).

    THE ORDER OF CHECKS IS LOAD-BEARING HERE.  This test is not marked gpu, so it also runs where a device is present, and it hands HOST
    pointers to entry points that take device memory (the forcing calls, the sort and staleness calls, permute_step_arrays).  That is
    safe only while nmp_host::check_index_block stays the first statement of each entry point, ahead of ensure_init() and of every other
    check: whoever moves it must move these cases to device memory or drop them."""
    lib = abi.load_library()
    p = _Poisoned()
    call, extra = _entries(lib, p)[entry]
    init = entry == "noahmp_hip_init"
    n = 0
    for over, bound in RULES_ALL + extra:
        if init:                                  # NOAHMP_INIT's tile ends at itf = min(ite, ide-1), jtf = min(jte, jde-1)
            bound = {"ite": "itf", "jte": "jtf"}.get(bound, bound)
        rc = call(p.args(p.s, **over))
        msg = lib.noahmp_hip_last_error().decode()
        assert rc == -103, (entry, over, rc, msg)
        assert msg.startswith(entry + ": index block refused, " + bound + ":"), (entry, over, msg)
        p.untouched()
        n += 1
    assert n >= len(RULES_ALL)
    if init:                                      # ... so a tile that leaves the memory block beyond the domain's last cell is none
        rc = call(p.args(p.s, ite=7, ide=8))
        assert rc == -103 and "itf" in lib.noahmp_hip_last_error().decode()
        p.untouched()


def test_c5_named_cases():
    """The cases the issue names, spelt out: forcing_prep with kms:kme = 0:1 (the old `nka < 2` guard let it through: level 2 was written
    into slot 0 of the next memory row) and 2:3; the step with kme = 1, with kts = kme and with ite = ime + 1."""
    lib = abi.load_library()
    p = _Poisoned()
    e = _entries(lib, p)
    for name, over in (("noahmp_hip_forcing_prep", dict(kms=0, kme=1)), ("noahmp_hip_forcing_prep", dict(kms=2, kme=3)),
                       ("noahmp_hip_step", dict(kme=1)), ("noahmp_hip_step", dict(kts=2, kme=2)), ("noahmp_hip_step", dict(ite=7, ime=6))):
        assert e[name][0](p.args(p.s, **over)) == -103, (name, over)
        assert name in lib.noahmp_hip_last_error().decode()
        p.untouched()


# ---------------------------------------------------------------------------------------------------------------- G1-G7: the device
def _generic(engine, on):
    engine.set_option("fixed_option_kernels", 0 if on else 1)
    engine.set_option("jit_option_kernels", 0 if on else 1)


def _device_step(engine, block, want, what, run=None):
    d = block.to_device("cuda:0")
    if run is None:
        st = engine.noahmplsm(d, 1, YR, JULIAN)
        assert st.code == 0 and st.n_skipped == 3, (what, st.code, st.n_skipped)
    else:
        run(d)
    assert_bits(d.to_host(), want, what)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_g1_step_device_memory(engine, compact, stepped, case):
    """Device-resident arrays: the generic kernel at block 64 / 256 with and without LDS, the ahead-of-time kernel of the default
    options (DVEG 3, RUN 1); E5 also through noahmp_hip_step_async + sync."""
    assert engine.exact_libm
    e = embed(compact, **CASES[case])
    want = place(e.copy(), stepped)
    prev = (engine.set_option("block", 256), engine.set_option("lds", 1))
    try:
        _generic(engine, True)
        for block in (64, 256):
            for lds in (0, 1):
                engine.set_option("block", block)
                engine.set_option("lds", lds)
                _device_step(engine, e, want, "generic kernel block %d lds %d %s" % (block, lds, case))
        _generic(engine, False)
        engine.set_option("block", prev[0])
        engine.set_option("lds", prev[1])
        _device_step(engine, e, want, "ahead-of-time kernel " + case)
        if case == "E5":
            def run(d):
                engine.noahmplsm_async(d.step_args(1, YR, JULIAN))
                st, step = engine.sync()
                assert (st.code, step, st.n_skipped) == (0, -1, 3)
            _device_step(engine, e, want, "step_async " + case, run)
    finally:
        _generic(engine, False)
        engine.set_option("block", prev[0])
        engine.set_option("lds", prev[1])


@pytest.mark.gpu
def test_g1_step_device_memory_kts2_block(engine, port, compact):
    """E7 (level 1 of the pressure differs from level kts) against the oracle on the same block: the generic kernel at both block sizes
    with and without LDS, the ahead-of-time kernel, the asynchronous step."""
    e = embed(compact, **E7)
    want = e.copy()
    assert port.noahmplsm(want, 1, YR, JULIAN).code == 0

    def run(what, step=None):
        d = e.to_device("cuda:0")
        if step is None:
            assert engine.noahmplsm(d, 1, YR, JULIAN).code == 0
        else:
            step(d)
        _assert_block_equal(d.to_host(), want, what + " E7")

    def async_step(d):
        engine.noahmplsm_async(d.step_args(1, YR, JULIAN))
        st, step = engine.sync()
        assert (st.code, step) == (0, -1)
    prev = (engine.set_option("block", 256), engine.set_option("lds", 1))
    try:
        _generic(engine, True)
        for block in (64, 256):
            for lds in (0, 1):
                engine.set_option("block", block)
                engine.set_option("lds", lds)
                run("generic kernel block %d lds %d" % (block, lds))
        _generic(engine, False)
        engine.set_option("block", prev[0])
        engine.set_option("lds", prev[1])
        run("ahead-of-time kernel")
        run("step_async", async_step)
    finally:
        _generic(engine, False)
        engine.set_option("block", prev[0])
        engine.set_option("lds", prev[1])


@pytest.mark.gpu
def test_g1_step_runtime_compiled_kernel(engine, port):
    """E5 with an option set that has no ahead-of-time kernel (one of test_runtime_compiled_kernels_bit_identical's, so the on-disk
    cache of the build serves it)."""
    cfg = ModelConfig(idveg=2, iopt_run=3, iopt_stc=2, iopt_frz=2)
    c = compact_store(cfg=cfg)
    want_c = c.copy()
    assert port.noahmplsm(want_c, 1, YR, JULIAN).code == 0
    e = embed(c, **CASES["E5"])
    assert engine.set_option("jit_option_kernels", -1) == 1
    _device_step(engine, e, place(e.copy(), want_c), "run-time compiled kernel E5")
    assert "generic kernel used" not in engine.lib.noahmp_hip_last_error().decode()
    d, compiled, hits, fallbacks = engine.jit_cache_info()
    assert compiled + hits >= 1 and fallbacks == 0, (d, compiled, hits, fallbacks)


@pytest.mark.gpu
def test_g2_step_host_memory_single_shot(engine, compact, stepped):
    e = embed(compact, **CASES["E5"])
    want = place(e.copy(), stepped)
    st = engine.noahmplsm(e, 1, YR, JULIAN)
    assert st.code == 0 and st.n_skipped == 3
    assert engine.set_option("last_host_path", -1) == 1              # single-shot staging
    assert_bits(e, want, "host memory, bounce buffers, E5")


@pytest.mark.gpu
def test_g2_step_host_memory_row_chunks(engine, port):
    """The row-chunk pipeline (page-locked arrays, >= 32768 columns, from the second call on): a 256 x 128 tile in an E5-shaped block,
    three calls on the same arrays against three oracle steps on the compact store."""
    c = compact_store(ni=256, nj=128, seed=4)
    want_c = c.copy()
    for it in (1, 2, 3):
        assert port.noahmplsm(want_c, it, YR, JULIAN).code == 0
    e = embed(c, **CASES["E5"])
    want = place(e.copy(), want_c)
    prev = {k: engine.set_option(k, v) for k, v in (("pin_host_arrays", 1), ("trust_out_mirror", 0))}
    try:
        for it in (1, 2, 3):
            assert engine.noahmplsm(e, it, YR, JULIAN).code == 0
            assert engine.set_option("last_host_path", -1) == (1 if it == 1 else 2), it      # calls 2 and 3 ran in row chunks
        assert engine.lib.noahmp_hip_debug_live_host_registrations() > 100
    finally:
        for k, v in prev.items():
            engine.set_option(k, v)
    assert_bits(e, want, "host memory, row chunks, E5-shaped 256 x 128")


RES_OPTS = ("resident_state", "lazy_download", "static_inputs")


def _two_resident_steps(engine, block, sorted_set=False, path=3):
    """Two calls on the same host arrays with the forcing rewritten in between, then fetch.  path: what "last_host_path" must say after
    either call (3: the tile-order mirrors, 4: the sorted mirror set)."""
    opts = RES_OPTS + (("resident_sorted",) if sorted_set else ())
    idx = block.index()
    jsl, isl = tile_slices(idx)
    try:
        for k in opts:
            engine.set_option(k, 1)
        assert engine.noahmplsm(block, 1, YR, JULIAN).code == 0
        assert engine.set_option("last_host_path", -1) == path
        second_forcing(block, jsl, isl, idx)
        assert engine.noahmplsm(block, 2, YR, JULIAN).code == 0
        assert engine.set_option("last_host_path", -1) == path
        engine.fetch()
    finally:
        for k in reversed(opts):
            engine.set_option(k, 0)


def second_forcing(s, jsl=slice(None), isl=slice(None), idx=None):
    """The forcing of the second step, written into level 1 (levels kts, kts+1 of the pressure) of the tile only."""
    k1 = 1 - idx["kms"] if idx else 0
    kp = idx["kts"] - idx["kms"] if idx else 0
    for k, f in (("t3d", 1.004), ("qv3d", 0.93), ("u_phy", 1.2), ("v_phy", 0.8)):
        s.a[k][jsl, k1, isl] = (s.a[k][jsl, k1, isl] * F(f)).astype(F)
    for slot in (kp, kp + 1):
        s.a["p8w3d"][jsl, slot, isl] = (s.a["p8w3d"][jsl, slot, isl] * F(0.997)).astype(F)
    for k, f in (("swdown", 0.6), ("glw", 1.05), ("coszin", 0.7)):
        s.a[k][jsl, isl] = (s.a[k][jsl, isl] * F(f)).astype(F)
    s.a["rainbl"][jsl, isl] = F(0.4)


@pytest.fixture(scope="module")
def two_steps(port):
    """Two oracle steps on compact stores (35 x 5 and 64 x 8) with second_forcing between them."""
    out = {}
    for ni, nj in ((NI, NJ), (64, 8)):
        c = compact_store(ni=ni, nj=nj)
        s = c.copy()
        assert port.noahmplsm(s, 1, YR, JULIAN).code == 0
        second_forcing(s)
        assert port.noahmplsm(s, 2, YR, JULIAN).code == 0
        out[(ni, nj)] = (c, s)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [0, 1], ids=["pageable", "page_locked"])
@pytest.mark.parametrize("kk", [(0, 4), (1, 5)], ids=["k0_4", "k1_5"])
def test_g3_resident_host_path(engine, two_steps, kk, pinned):
    """resident_state + lazy_download + static_inputs: the second call uploads only level 1 of T3D / QV3D / U_PHY / V_PHY (page-locked
    arrays: one strided copy per array at offset k1; pageable ones: every level through the bounce buffers) -- E5's halo and origin."""
    c, want_c = two_steps[(NI, NJ)]
    g = dict(CASES["E5"], kms=kk[0], kme=kk[1])
    e = embed(c, **g)
    before = e.copy()
    second_forcing(before, *tile_slices(e.index()), e.index())
    prev = engine.set_option("pin_host_arrays", pinned)
    try:
        _two_resident_steps(engine, e)       # "pin_host_arrays": the arrays are page-locked when they show up the second time
        if pinned:
            assert engine.lib.noahmp_hip_debug_live_host_registrations() > 100
    finally:
        engine.set_option("pin_host_arrays", prev)
    assert_bits(e, place(before, want_c), "resident host path kms:kme = %d:%d pinned %d" % (kk[0], kk[1], pinned))


@pytest.mark.gpu
@pytest.mark.parametrize("kk", [(1, 5), (0, 4)], ids=["k1_5_sorted", "k0_4_declined"])
def test_g3_resident_sorted(engine, two_steps, kk):
    """resident_sorted with memory == tile (64 x 8): kms = 1 runs on the sorted mirror set, kms = 0 must decline it (its exchange moves
    memory level 0); either way the bits of the oracle's two steps."""
    c, want_c = two_steps[(64, 8)]
    e = embed(c, halo=(0, 0, 0, 0), kms=kk[0], kme=kk[1])
    before = e.copy()
    second_forcing(before, *tile_slices(e.index()), e.index())
    _two_resident_steps(engine, e, sorted_set=True, path=4 if kk[0] == 1 else 3)
    assert_bits(e, place(before, want_c), "resident_sorted kms:kme = %d:%d" % kk)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["E1", "E2"])
def test_g4_sorted_device_store(engine, port, case):
    """Engine.sort_store(tair=True) takes its temperature bins from level 1 of T3D: the permutation of a block with kme > 2 / kms = 0 is
    that of the compact store, and one step on the sorted block (the class ranges in one launch) is the oracle's, permuted."""
    c = compact_store(ni=64, nj=8)
    want_c = c.copy()
    assert port.noahmplsm(want_c, 1, YR, JULIAN).code == 0
    dc = c.to_device("cuda:0")
    perm_c = engine.sort_store(dc, tair=True).cpu().numpy()
    g = dict(CASES[case])
    e = embed(c, **g)
    d = e.to_device("cuda:0")
    perm = engine.sort_store(d, tair=True).cpu().numpy()
    assert np.array_equal(perm, perm_c) and not np.array_equal(perm, np.arange(perm.size))
    assert d.class_ranges == dc.class_ranges and d.class_ranges[0] > 300
    st = engine.noahmplsm(d, 1, YR, JULIAN)
    engine._apply_ranges(None)
    assert st.code == 0 and (st.n_land, st.n_glacier) == d.class_ranges
    got = d.to_host()
    bad = []
    for k, y in want_c.a.items():
        if k == "dzs" or k in ATM:
            continue
        y = y.transpose(0, 2, 1).reshape(-1, y.shape[1])[perm] if y.ndim == 3 else y.reshape(-1)[perm]
        x = got.a[k]
        x = x.transpose(0, 2, 1).reshape(-1, x.shape[1]) if x.ndim == 3 else x.reshape(-1)
        if not np.array_equal(words(x), words(y)):
            bad.append(k)
    assert not bad, "sorted step %s: %s differ from the oracle, permuted" % (case, bad)


def _dev(d):
    import torch
    return {k: (torch.from_numpy(v).cuda() if v is not None else None) for k, v in d.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL[:5])
def test_g5_forcing(engine, port, compact, forcing_ref, case):
    import torch

    def interpolate(s, ra, rb, rain):
        d = s.to_device("cuda:0")
        rd = torch.from_numpy(rain).cuda()
        engine.forcing_interpolate(d, _dev(ra), _dev(rb), IDTS, IDTS2, rd)
        rain[...] = rd.cpu().numpy()
        s.a = d.to_host().a

    def prep(s, lon, rain):
        d = s.to_device("cuda:0")
        jul = engine.forcing_prep(d, torch.from_numpy(lon).cuda(), torch.from_numpy(rain).cuda(), *WHEN, scale_vegfra=True, first_step=True)
        assert jul == forcing_ref["julian"]
        s.a = d.to_host().a
    _check_forcing(interpolate, prep, compact, forcing_ref, case, "device")
    # the two in one launch: the final state of the sequence, and the same as the oracle on the same block
    e, ra, rb, lon, rain, frain = _forcing_block(compact, forcing_ref, case)
    before = e.copy()
    o, orain = e.copy(), np.array(rain, copy=True)
    port.forcing_interpolate(o, ra, rb, IDTS, IDTS2, orain)
    port.forcing_prep(o, lon, orain, *WHEN, scale_vegfra=True, first_step=True)
    d = e.to_device("cuda:0")
    rd = torch.from_numpy(rain).cuda()
    jul = engine.forcing_interpolate_prep(d, _dev(ra), _dev(rb), IDTS, IDTS2, rd, torch.from_numpy(lon).cuda(), *WHEN, scale_vegfra=True,
                                          first_step=True)
    assert jul == forcing_ref["julian"]
    got = d.to_host()
    want = place(place(before, forcing_ref["interp"], LEV1), forcing_ref["prep"], LEV12)
    planes = [("rain_rate", rd.cpu().numpy(), embed_plane(forcing_ref["rain"], frain, e.index()))]
    assert_bits(got, want, "device forcing_interpolate_prep " + case, LEV12, planes=planes)
    _assert_block_equal(got, o, "device forcing_interpolate_prep vs the oracle on the same block " + case)
    assert np.array_equal(words(planes[0][1]), words(orain))


@pytest.mark.gpu
def test_g6_cold_start(engine, port, compact):
    def call(a, iswater, st):
        # `a` points at host arrays: the host-memory path of noahmp_hip_init
        return engine.lib.noahmp_hip_init(C.byref(a), iswater, 1, abi.MEM_HOST, None, C.byref(st))
    _check_init(call, port, compact)
    # device-resident arrays
    for name, c, e, bump_c, bump_e in _init_pairs(compact):
        want_c = c.copy()
        _run_init(lambda a, st: port.lib.nmp_oracle_init(C.byref(a), c.cfg.iswater, 1, C.byref(st)), want_c, bump_c)
        d = e.to_device("cuda:0")
        _run_init(lambda a, st: engine.lib.noahmp_hip_init(C.byref(a), e.cfg.iswater, 1, abi.MEM_DEVICE, None, C.byref(st)), d, bump_e)
        assert_bits(d.to_host(), place(e.copy(), want_c), "noahmp_init, device memory " + name)


GW_TILES = [(1, 1), (63, 3), (64, 4), (65, 5), (130, 9), (254, 2), (255, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("tile", GW_TILES, ids=lambda t: "%dx%d" % t)
def test_g7_groundwater(engine, port, tile):
    """WTABLE_mmf_noahmp, its split form and GROUNDWATER_INIT with a memory ring wider than the stencil needs (3 cells), a shifted origin,
    the domain's edge on the west and south sides only, at tile sizes around the edges of the 64 x 4, 64 x 8 and 256-cell tilings:
    the oracle on the same block, and the split form equal to the whole call."""
    import torch
    ni, nj = tile
    c = compact_store(ni=ni, nj=nj, seed=4, cfg=ModelConfig(iopt_run=5), groundwater=True)
    its, jts = 12, -7
    e = embed(c, halo=(3, 3, 3, 3), kms=0, kme=3, origin=(its, jts), domain=(its, its + ni + 40, jts, jts + nj + 40))
    want = e.copy()
    port.wtable_mmf(want)
    d = e.to_device("cuda:0")
    engine.wtable_mmf(d)
    _assert_block_equal(d.to_host(), want, "wtable_mmf %dx%d" % tile)
    if ni * nj > 1:
        assert not np.array_equal(words(want.a["zwtxy"]), words(e.a["zwtxy"]))
    d = e.to_device("cuda:0")
    qlat = torch.full((e.nj, e.ni), 7.0, dtype=torch.float32, device="cuda:0")
    w = d.wtable_args()
    engine.wtable_lateral_async(w, qlat)
    engine.wtable_columns_async(w, qlat)
    engine.stream_sync()
    _assert_block_equal(d.to_host(), want, "wtable_lateral + wtable_columns %dx%d" % tile)
    q = qlat.cpu().numpy()
    jsl, isl = tile_slices(e.index())
    halo = np.ones(q.shape, bool)
    halo[jsl, isl] = False
    assert (q[halo] == 7.0).all()                          # QLAT is written on the tile only
    want = e.copy()
    port.groundwater_init(want)
    d = e.to_device("cuda:0")
    engine.groundwater_init(d)
    _assert_block_equal(d.to_host(), want, "groundwater_init %dx%d" % tile)
