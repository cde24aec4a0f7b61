"""GPU parity tests (run with -m gpu on an MI355X): the HIP engine, called through the C-ABI,
against the oracle (C restatement, itself bit-exact to the reference) and against the golden
vectors the reference produced.  Tolerances: tools/compare.py (per-variable TIGHT tolerance for
>= 97 % of the entries + a hard ENVELOPE for all of them; floor = the reference's own -O0/-O2
reproducibility)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_store
from golden import npz_parts
from noahmp_amd import synth
from noahmp_amd.abi import FIELD_INFO
from noahmp_amd.state import ModelConfig
from tools.compare import parity_check, exact_check

pytestmark = pytest.mark.gpu

EXACT = None


def _exact(engine):
    """True for the shipped build (reference-libm algorithms on the device: bit-identity is asserted).  A library built with
    -DNMP_EXACT_LIBM=0 (ocml) only meets the statistical contract; the suite refuses to downgrade silently: such a build must
    be announced with NMP_TEST_OCML_BUILD=1."""
    global EXACT
    if EXACT is None:
        EXACT = engine.exact_libm
        if not EXACT and os.environ.get("NMP_TEST_OCML_BUILD") != "1":
            raise AssertionError("libnoahmp_hip.so was built without the reference-libm restatements (exact_libm = 0): the bit-identity "
                                 "tests would silently turn into statistical ones.  Set NMP_TEST_OCML_BUILD=1 to test such a build.")
    return EXACT


def _check(ref, test, engine=None, allow_cols=0, **kw):
    """Default build (reference libm algorithms on the device): results are BIT-IDENTICAL to the oracle.
    ocml build (NMP_EXACT_LIBM=0): per-variable tolerance + envelope of tools/compare.py."""
    if engine is None or _exact(engine):
        ok, lines = exact_check(ref, test, fields=kw.get("fields"), skip=kw.get("skip", ()), allow_cols=allow_cols)
    else:
        ok, lines = parity_check(ref, test, **kw)
    assert ok, "\n".join(lines)


def _outs(store):
    return [k for k in store.a if FIELD_INFO[k][2] != "in"]


def test_config1_single_column_trajectory(engine):
    """BASELINE config 1 (the reference's CPU-runnable case): 24 hourly steps vs the reference run."""
    g = np.load(os.path.join(GOLDEN, "golden_config1.npz"))
    s = load_store(g, "init", 1, 1)
    d = s.to_device("cuda:0")
    for it in range(1, 25):
        synth.diurnal_forcing(s, (it - 1) % 24)
        for k in ("coszin", "swdown", "glw", "t3d", "rainbl"):
            d.a[k].copy_(__import__("torch").from_numpy(s.a[k]))
        st = engine.noahmplsm(d, it, 2000, 180.0)
        assert st.code == 0 and st.n_land == 1
    h = d.to_host()
    ref = load_store({("x/%s" % k): g["traj/%s" % k][23] for k in s.a}, "x", 1, 1)
    if _exact(engine):
        _check(ref, h, engine)                       # 24 free-running steps: still the reference's bits
    else:
        for k in ("tslb", "smois", "sh2o"):
            np.testing.assert_allclose(h.a[k], ref.a[k], rtol=5e-5, atol=1e-5, err_msg=k)
        ok, lines = parity_check(ref, h, steps=24, frac=1.0)
        assert ok, "\n".join(lines)


def test_mixed_tile_single_step_restart_vs_oracle(engine, port, tables):
    """Each of 24 steps: HIP starts from the oracle's state, compared after one step."""
    s = synth.mixed_small(tables[1], ni=64, nj=8)
    synth.first_step_fixups(s)
    so = s.copy()
    seen = set()
    for it in range(1, 25):
        synth.diurnal_forcing(so, (it - 1) % 24, t_offset=s.t_offset)
        sd = so.copy()
        port.noahmplsm(so, it, 2000, 180.0)
        st = engine.noahmplsm(sd, it, 2000, 180.0)          # host-memory path of the C-ABI
        assert st.code == 0 and st.n_land + st.n_glacier == 512 and st.n_glacier > 0
        _check(so, sd, engine, steps=1)
        seen.update(np.unique(so["isnowxy"]).tolist())
    assert seen == {0, -1, -2, -3}


def test_mixed_tile_free_run_vs_golden(engine):
    """24-step free run on the device-resident path vs the reference's snapshots (steps 1/12/24)."""
    import torch
    g = np.load(os.path.join(GOLDEN, "golden_mixed.npz"))
    s = load_store(g, "init", 64, 4)
    toff = g["t_offset"]
    d = s.to_device("cuda:0")
    for it in range(1, 25):
        synth.diurnal_forcing(s, (it - 1) % 24, t_offset=toff)
        for k in ("coszin", "swdown", "glw", "t3d", "rainbl"):
            d.a[k].copy_(torch.from_numpy(s.a[k]))
        st = engine.noahmplsm(d, it, 2000, 180.0)
        assert st.code == 0
        if it in (1, 12, 24):
            ref = load_store(g, "step%02d" % it, 64, 4)
            _check(ref, d.to_host(), engine, steps=it, fields=_outs(ref))


def test_option_sweep_vs_golden(engine):
    """Every OPT_* alternative (22 option sets), one step at noon, vs the reference."""
    g = npz_parts.load(os.path.join(GOLDEN, "golden_opts.npz"))
    sweep = [eval(x) for x in g["sweep"]]
    base = load_store(g, "init", 32, 4)
    for n, kw in enumerate(sweep):
        s = base.copy()
        s.cfg = ModelConfig(**kw)
        if kw.get("iopt_run") == 5:
            s["waxy"] = 0.0
            s["wtxy"] = 0.0
        st = engine.noahmplsm(s, 1, 2000, 180.0)
        assert st.code == 0, kw
        ref = load_store(g, "opt%02d" % n, 32, 4)
        skip = ("t2mvxy", "t2mbxy", "q2mvxy", "q2mbxy", "chv2xy", "chb2xy") if kw.get("iopt_sfc") == 2 else ()
        if _exact(engine):
            ok, lines = exact_check(ref, s, fields=_outs(ref), skip=skip)
        else:
            ok, lines = parity_check(ref, s, steps=1, fields=_outs(ref), skip=skip, frac=0.05)
        assert ok, "%s\n%s" % (kw, "\n".join(lines))


def test_host_and_device_paths_bit_identical(engine, tables):
    s = synth.mixed_small(tables[1], ni=64, nj=4)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 13, t_offset=s.t_offset)
    h = s.copy()
    d = s.to_device("cuda:0")
    engine.noahmplsm(h, 1, 2000, 180.0)
    engine.noahmplsm(d, 1, 2000, 180.0)
    dh = d.to_host()
    for k in _outs(h):
        np.testing.assert_array_equal(h.a[k], dh.a[k], err_msg=k)


def test_launch_variants_bit_identical(engine, tables):
    """Block size and LDS-vs-scratch layer storage change scheduling only, never results."""
    s = synth.mixed_small(tables[1], ni=64, nj=8)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 11, t_offset=s.t_offset)
    outs = []
    try:
        for block, lds in ((64, 1), (64, 0), (128, 1), (256, 1), (256, 0)):
            engine.set_option("block", block)
            engine.set_option("lds", lds)
            x = s.copy()
            engine.noahmplsm(x, 1, 2000, 180.0)
            outs.append(x)
    finally:
        engine.set_option("block", 256)
        engine.set_option("lds", 1)
    for x in outs[1:]:
        for k in _outs(x):
            np.testing.assert_array_equal(outs[0].a[k], x.a[k], err_msg=k)


def test_tile_split_invariance(engine, tables):
    """its/ite/jts/jte sub-tiles of a larger memory block give the same columns as the whole tile."""
    import ctypes as C
    from noahmp_amd import abi
    s = synth.mixed_small(tables[1], ni=48, nj=6)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    whole = s.copy()
    engine.noahmplsm(whole, 2, 2000, 180.0)
    parts = s.copy()
    for (i0, i1, j0, j1) in ((1, 20, 1, 6), (21, 48, 1, 3), (21, 48, 4, 6)):
        a = parts.step_args(2, 2000, 180.0)
        a.its, a.ite, a.jts, a.jte = i0, i1, j0, j1
        st = abi.Status()
        rc = engine.lib.noahmp_hip_step(C.byref(a), abi.MEM_HOST, None, C.byref(st))
        assert rc == 0 and st.n_land + st.n_glacier == (i1 - i0 + 1) * (j1 - j0 + 1)
    for k in _outs(whole):
        np.testing.assert_array_equal(whole.a[k], parts.a[k], err_msg=k)


def test_empty_and_one_cell_tiles(engine, tables):
    """A rank whose tile is empty (ite < its or jte < jts: more ranks than rows) advances nothing and touches nothing; a one-cell tile
    in a corner of the memory block advances exactly that column -- host and device arrays, synchronous and asynchronous call."""
    import ctypes as C
    from noahmp_amd import abi
    s = synth.mixed_small(tables[1], ni=48, nj=6)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    whole = s.copy()
    engine.noahmplsm(whole, 2, 2000, 180.0)
    for mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        work = s.copy()
        blk = work if mem == abi.MEM_HOST else work.to_device("cuda:0")
        for (i0, i1, j0, j1) in ((5, 4, 1, 6), (1, 48, 3, 2)):                  # empty in i, empty in j
            a = blk.step_args(2, 2000, 180.0)
            a.its, a.ite, a.jts, a.jte = i0, i1, j0, j1
            st = abi.Status()
            assert engine.lib.noahmp_hip_step(C.byref(a), mem, None, C.byref(st)) == 0
            assert (st.n_land, st.n_glacier, st.n_skipped, st.code) == (0, 0, 0, 0)
            if mem == abi.MEM_DEVICE:                                            # (the asynchronous call takes device arrays only)
                assert engine.lib.noahmp_hip_step_async(C.byref(a), None) == 0
                st2, _ = engine.sync()
                assert (st2.n_land, st2.n_glacier, st2.code, st2.kernel_ms) == (0, 0, 0, 0.0)
        got = work if mem == abi.MEM_HOST else blk.to_host()
        for k in _outs(whole):
            np.testing.assert_array_equal(got.a[k], s.a[k], err_msg=k)          # nothing was touched
        a = blk.step_args(2, 2000, 180.0)
        a.its, a.ite, a.jts, a.jte = 48, 48, 6, 6                               # the last cell of the block
        st = abi.Status()
        assert engine.lib.noahmp_hip_step(C.byref(a), mem, None, C.byref(st)) == 0
        assert st.n_land + st.n_glacier + st.n_skipped == 1
        got = work if mem == abi.MEM_HOST else blk.to_host()
        for k in _outs(whole):
            x, y, z = got.a[k], whole.a[k], s.a[k]
            np.testing.assert_array_equal(x[-1, ..., -1], y[-1, ..., -1], err_msg=k)
            m = np.ones(x.shape, bool)
            m[-1, ..., -1] = False
            np.testing.assert_array_equal(x[m], z[m], err_msg=k)


def test_permutation_invariance_large(engine, tables):
    """Size-independent property at 262 144 columns: columns are independent, so permuting them
    permutes the results bit-for-bit (catches any cross-column / indexing / race error)."""
    s = synth.config3(tables[1], ni=512, nj=512, seed=9)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    rng = np.random.Generator(np.random.Philox(1))
    perm = rng.permutation(s.ncol)
    p = s.copy()
    for k, v in s.a.items():
        if k == "dzs":
            continue
        if v.ndim == 2:
            p.a[k][...] = v.reshape(-1)[perm].reshape(v.shape)
        else:
            nj, nk, ni = v.shape
            flat = v.transpose(0, 2, 1).reshape(-1, nk)[perm]
            p.a[k][...] = flat.reshape(nj, ni, nk).transpose(0, 2, 1)
    st = engine.noahmplsm(s, 3, 2000, 180.0)
    st2 = engine.noahmplsm(p, 3, 2000, 180.0)
    assert st.code == 0 and st2.code == 0 and st.n_land == st2.n_land and st.n_land + st.n_glacier == s.ncol
    for k in _outs(s):
        v, w = s.a[k], p.a[k]
        if v.ndim == 2:
            np.testing.assert_array_equal(v.reshape(-1)[perm], w.reshape(-1), err_msg=k)
        else:
            nj, nk, ni = v.shape
            np.testing.assert_array_equal(v.transpose(0, 2, 1).reshape(-1, nk)[perm],
                                          w.transpose(0, 2, 1).reshape(-1, nk), err_msg=k)


def test_full_size_conservation_config2(engine, tables):
    """BASELINE config 2 at full size (1 048 576 columns), 3 device-resident steps: the in-model
    SW / energy / water balance checks (lsm:1164-1222) hold for every column (status 0), the state
    stays finite, and a 4096-column sample agrees with the oracle."""
    s = synth.config2(tables[1])
    synth.first_step_fixups(s)
    d = s.to_device("cuda:0")
    import torch
    for it in range(1, 4):
        synth.diurnal_forcing(s, 10 + it, t_offset=s.t_offset)
        for k in ("coszin", "swdown", "glw", "t3d", "rainbl"):
            d.a[k].copy_(torch.from_numpy(s.a[k]))
        st = engine.noahmplsm(d, it, 2000, 180.0)
        assert st.code == 0 and st.n_land == 1024 * 1024
    for k in ("tsk", "hfx", "lh", "tslb", "smois", "snow"):
        assert bool(torch.isfinite(d.a[k]).all()), k
    assert float(d.a["tslb"].min()) > 240.0 and float(d.a["tslb"].max()) < 330.0
    assert float(d.a["smois"].min()) > 0.0 and float(d.a["smois"].max()) <= 0.5


def test_full_size_config2_bit_identical_to_oracle(engine, port, tables):
    """BASELINE config 2 at its full size, one noon step: all 1 048 576 columns x every output field carry
    the oracle's (= the reference's) bits."""
    if not _exact(engine):
        pytest.skip("ocml build: statistical parity only")
    s = synth.config2(tables[1])
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    so = s.copy()
    port.noahmplsm(so, 1, 2000, 180.0)
    st = engine.noahmplsm(s, 1, 2000, 180.0)
    assert st.code == 0 and st.n_land == 1024 * 1024
    _check(so, s, engine)        # EXP is pinned on both sides (oracle/nmp_pin_expf.c): no column may differ


def test_sample_of_config2_vs_oracle(engine, port, tables):
    s = synth.config2(tables[1], ni=256, nj=16)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    so, sd = s.copy(), s.copy()
    port.noahmplsm(so, 1, 2000, 180.0)
    engine.noahmplsm(sd, 1, 2000, 180.0)
    _check(so, sd, engine, steps=1)


def test_error_channel_first_column_wins(engine, tables):
    """A fatal column is reported with its Fortran (i,j); lowest linear index wins; others advance."""
    from noahmp_amd.driver import NoahMPFatal
    s = synth.mixed_small(tables[1], ni=32, nj=4)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    s["isltyp"][2, 7] = 25          # REDPRM: too many input soil types (lsm:9266)
    s["ivgtyp"][3, 1] = 40          # REDPRM: too many input landuse types (lsm:9272)
    before = s.copy()
    with pytest.raises(NoahMPFatal) as e:
        engine.noahmplsm(s, 1, 2000, 180.0)
    assert (e.value.code, e.value.i, e.value.j) == (1, 8, 3)
    assert s["tsk"][2, 7] == before["tsk"][2, 7]            # offending column left untouched
    assert (s["tsk"][0] != before["tsk"][0]).all()          # the rest advanced


def test_isnow_out_of_range_is_reported(engine, tables):
    """ISNOWXY outside -NSNOW..0 (the reference would index its layer arrays out of bounds) is a reported error at that column,
    which is left untouched; the other columns advance."""
    from noahmp_amd.driver import NoahMPFatal
    s = synth.mixed_small(tables[1], ni=32, nj=4)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    s["isnowxy"][1, 5] = -7
    s["isnowxy"][3, 9] = 2
    before = s.copy()
    with pytest.raises(NoahMPFatal) as e:
        engine.noahmplsm(s, 1, 2000, 180.0)
    assert (e.value.code, e.value.i, e.value.j) == (18, 6, 2)
    assert engine.lib.noahmp_hip_error_string(18).decode().startswith("ISNOWXY")
    assert s["tsk"][1, 5] == before["tsk"][1, 5] and s["isnowxy"][1, 5] == -7
    assert (s["tsk"][0] != before["tsk"][0]).all()


def test_water_and_seaice_points(engine, port, tables):
    s = synth.mixed_small(tables[1], ni=16, nj=2)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    s["xland"][0, 0] = 2.0
    s["xice"][0, 1] = 1.0
    so, sd = s.copy(), s.copy()
    port.noahmplsm(so, 1, 2000, 180.0)       # itimestep 1: exercises the water-point init too
    st = engine.noahmplsm(sd, 1, 2000, 180.0)
    assert st.n_skipped == 2 and st.n_land + st.n_glacier == 30
    for k in ("smois", "tslb", "sh2o", "xlaixy", "smstav"):
        np.testing.assert_array_equal(so.a[k][..., :2], sd.a[k][..., :2], err_msg=k)


def test_unsupported_options_are_rejected(engine, tables):
    from noahmp_amd.driver import NoahMPFatal
    s = synth.mixed_small(tables[1], ni=8, nj=1)
    s.cfg = ModelConfig(iopt_sfc=3)
    with pytest.raises(NoahMPFatal) as e:
        engine.noahmplsm(s, 1, 2000, 180.0)
    assert e.value.code == 11


# ------------------------------------------------------------------------------------------------
# MMF groundwater: noahmp_hip_wtable_mmf vs the oracle of WTABLE_mmf_noahmp (gw:14-606)
from test_groundwater import gw_store, GW_OUT, CASES  # noqa: E402

# The device differs from the oracle's glibc only in expf/powf (ocml, <= 1-2 ulp) feeding a few dozen
# float32 operations, so the deviations are ulp-level: rtol 5e-6.  QSLAT and RECH are sums of cancelling
# terms (8 stencil fluxes; recharge minus its clamps), so an ulp of a term is a larger relative error of the
# sum: they get an absolute allowance of 1e-4 of the field's rms on top.
GW_TOL = {n: (5e-6, 1e-7) for n in GW_OUT}
GW_TOL.update(qslat=(1e-5, 1e-4), rechxy=(1e-5, 1e-4), deeprechxy=(1e-5, 1e-4),
              qspring=(2e-5, 1e-5), qsprings=(2e-5, 1e-5))   # QSPRING = what is left after all capacities are subtracted


def _gw_close(ref, test, what="", engine=None):
    if engine is not None and _exact(engine):
        ok, lines = exact_check(ref, test, fields=GW_OUT)
        assert ok, what + "\n" + "\n".join(lines)
        return
    _gw_tol(ref, test, what)


def _gw_tol(ref, test, what=""):
    """ocml build only.  Every cell within 20x the tolerance; all but 1e-4 of the cells (at least 3) within the tolerance itself:
    the deep-recharge update (gw:147-161) subtracts two large fluxes and divides by the distance to the water
    table, which amplifies an ulp of powf by 10-100x in a handful of cells of the 1 m stress case."""
    for n in GW_OUT:
        x, y = ref.a[n].astype(np.float64), test.a[n].astype(np.float64)
        rtol, arms = GW_TOL[n]
        tol = rtol * np.abs(x) + arms * max(float(np.sqrt(np.mean(x * x))), 1e-30) + 1e-30
        d = np.abs(x - y)
        bad = ~(d <= tol)
        worse = ~(d <= 20 * tol)
        msg = "%s %s: %d cells out of tolerance (%d beyond 20x), worst |d|=%g at value %g" % (
            what, n, int(bad.sum()), int(worse.sum()), float(d[bad].max()) if bad.any() else 0.0,
            float(x[bad][d[bad].argmax()]) if bad.any() else 0.0)
        assert not worse.any(), msg
        assert bad.sum() <= max(3, 1e-4 * x.size), msg


@pytest.mark.parametrize("case", CASES, ids=lambda c: "stress%g_area%g" % (c["stress"], c["area"]))
def test_groundwater_vs_oracle(engine, port, tables, case):
    s0 = gw_store(tables, ni=256, nj=128, **case)
    a = s0.copy()
    for call in range(3):
        b = a.copy()                                  # the GPU restarts from the oracle's state each call
        so = port.wtable_mmf(a)
        sg = engine.wtable_mmf(b)
        assert sg.n_land == so.n_land and sg.n_skipped == so.n_skipped
        _gw_close(a, b, "call %d" % call, engine)
        a.a["deeprechxy"][...] = s0.a["deeprechxy"]


def test_groundwater_golden_fixture(engine):
    """The committed reference output (tests/golden/make_golden_gw.py, compiled reference)."""
    from noahmp_amd.state import ColumnStore
    z = np.load(os.path.join(GOLDEN, "golden_gw.npz"))
    ni, nj = int(z["ni"]), int(z["nj"])
    s = ColumnStore(ni, nj, ModelConfig(iopt_run=5)).add_groundwater()
    for k in s.a:
        if "in/" + k in z:
            s.a[k][...] = z["in/" + k]
    want = s.copy()
    for n in GW_OUT:
        want.a[n][...] = z["out/" + n]
    engine.wtable_mmf(s)
    _gw_close(want, s, "golden", engine)


def test_groundwater_host_and_device_paths_bit_identical(engine, tables):
    s = gw_store(tables, ni=96, nj=40, stress=0.02)
    h = s.copy()
    d = s.to_device("cuda:0")
    engine.wtable_mmf(h)
    engine.wtable_mmf(d)
    dh = d.to_host()
    for k in GW_OUT:
        np.testing.assert_array_equal(h.a[k], dh.a[k], err_msg=k)
    for k in ("fdepth", "topo", "eqwtd", "smoiseq", "isltyp"):       # IN planes are not written
        np.testing.assert_array_equal(s.a[k], dh.a[k], err_msg=k)


def _run_tiles(engine, s0, nproc):
    """Each 'rank' gets its tile + 1-cell ring cut from the global state (what exchange_halo delivers)."""
    from noahmp_amd.partition import tile_geometry
    from noahmp_amd.state import ColumnStore
    out = s0.copy()
    for rank in range(nproc):
        geo = tile_geometry(s0.ni, s0.nj, nproc, rank)
        ims, ime, jms, jme = geo["ims"], geo["ime"], geo["jms"], geo["jme"]
        its, ite, jts, jte = geo["its"], geo["ite"], geo["jts"], geo["jte"]
        loc = ColumnStore(ime - ims + 1, jme - jms + 1, s0.cfg).add_groundwater()
        for k in set(loc.a) & (set(GW_OUT) | {"fdepth", "topo", "isltyp", "ivgtyp", "xland", "xice", "area",
                                            "eqwtd", "rivercond", "riverbed", "pexp", "smoiseq"}):
            loc.a[k][...] = s0.a[k][jms - 1:jme, ..., ims - 1:ime]
        loc.set_index(**geo)
        engine.wtable_mmf(loc)
        for k in GW_OUT:
            out.a[k][jts - 1:jte, ..., its - 1:ite] = loc.a[k][jts - jms:jte - jms + 1, ..., its - ims:ite - ims + 1]
    return out


def test_groundwater_decomposition_invariance(engine, tables):
    """SURVEY 8e parity target: tiles with a ZWTXY ring reproduce the single-domain result bit for bit."""
    s0 = gw_store(tables, ni=101, nj=67, stress=0.02)
    whole = s0.copy()
    engine.wtable_mmf(whole)
    for nproc in (2, 4, 8):
        out = _run_tiles(engine, s0, nproc)
        for k in GW_OUT:
            np.testing.assert_array_equal(whole.a[k], out.a[k], err_msg="%s nproc=%d" % (k, nproc))


def test_groundwater_refuses_tile_without_ring(engine, tables):
    import ctypes as C
    from noahmp_amd import abi
    s = gw_store(tables, ni=32, nj=16)
    w = s.wtable_args()
    w.ids, w.ide = -10, 100                    # tile is interior to the domain but memory has no ring
    st = abi.Status()
    rc = engine.lib.noahmp_hip_wtable_mmf(C.byref(w), abi.MEM_HOST, None, C.byref(st))
    assert rc == -103 and b"ring" in engine.lib.noahmp_hip_last_error()


def test_groundwater_full_size_config4(engine, port, tables):
    """BASELINE config-4 grid (4608 x 1536 = 7.08 M cells): the whole field against the oracle, plus the
    8-rank (4 x 2, mpp rule) decomposition against the single domain, bit for bit."""
    from noahmp_amd.state import ColumnStore
    ni, nj = 4608, 1536
    cfg = ModelConfig(iopt_run=5)
    r = np.random.default_rng(44)
    s = ColumnStore(ni, nj, cfg).add_groundwater()
    a = s.a
    a["ivgtyp"][...] = synth.CONUS_VEG[r.integers(0, len(synth.CONUS_VEG), size=(nj, ni))]
    a["isltyp"][...] = r.integers(1, 13, size=(nj, ni)).astype(np.int32)
    a["xland"][...] = 1.0
    for k, sm in enumerate((0.25, 0.27, 0.30, 0.31)):
        a["smois"][:, k, :] = np.float32(sm) + r.uniform(-0.05, 0.05, size=(nj, ni)).astype(np.float32)
        a["sh2o"][:, k, :] = a["smois"][:, k, :] * np.float32(0.9)
    synth.groundwater_fields(s, tables[1], seed=45, stress=0.02)
    s.a = {k: s.a[k] for k in set(GW_OUT) | {"fdepth", "topo", "isltyp", "ivgtyp", "xland", "xice", "area", "eqwtd",
                                            "rivercond", "riverbed", "pexp", "smoiseq", "dzs"}}
    # (the planes the groundwater step never touches are dropped: 3 copies of 118 full-size fields is 10 GB)
    o = s.copy()
    g = s.copy()
    so = port.wtable_mmf(o)
    sg = engine.wtable_mmf(g)
    assert sg.n_land == so.n_land > 6_000_000
    _gw_close(o, g, "full size", engine)
    out = _run_tiles(engine, s, 8)
    for k in GW_OUT:
        np.testing.assert_array_equal(g.a[k], out.a[k], err_msg=k)


MIXES = [dict(), dict(idveg=2, iopt_run=3, iopt_stc=2),
         dict(iopt_sfc=2, iopt_crs=2, iopt_btr=2, iopt_frz=2, iopt_inf=2),
         dict(iopt_rad=1, iopt_alb=1, iopt_snf=3, iopt_tbot=1, idveg=5)]


@pytest.mark.parametrize("kw", MIXES, ids=[repr(k) for k in MIXES])
def test_free_run_option_mixes_bit_identical(engine, port, tables, kw):
    """36 free-running hourly steps of a 4096-column mixed tile under combined non-default options, device-resident,
    against the oracle advanced from the same start: every output, every step (tools/long_parity.py runs 96)."""
    if not _exact(engine):
        pytest.skip("ocml build: statistical parity only")
    import torch
    s = synth.mixed_small(tables[1], ni=128, nj=32, seed=31, cfg=ModelConfig(**kw))
    synth.first_step_fixups(s)
    o, d = s.copy(), s.to_device("cuda:0")
    for it in range(1, 37):
        synth.diurnal_forcing(o, (it - 1) % 24, t_offset=s.t_offset)
        for k in ("coszin", "swdown", "glw", "t3d", "rainbl"):
            d.a[k].copy_(torch.from_numpy(o.a[k]))
        so = port.noahmplsm(o, it, 2000, 180.0 + it / 24.0)
        sd = engine.noahmplsm(d, it, 2000, 180.0 + it / 24.0, check=False)
        assert so.code == sd.code == 0, (it, so.code, sd.code)
        if it % 6 == 0:
            ok, lines = exact_check(o, d.to_host())
            assert ok, "step %d\n%s" % (it, "\n".join(lines))
    assert set(np.unique(o.a["isnowxy"]).tolist()) == {0, -1, -2, -3}


def test_pageable_arrays_travel_through_the_engines_bounce_buffers(engine, tables):
    """Round 6 (nmp_stage.hpp): no pageable pointer of the caller reaches the HIP runtime -- arrays of several MiB each (the size from
    which the runtime would page-lock them in place) go through the engine's own page-locked bounce buffers, page-locked arrays are
    copied directly; either way the bits of the device path.  noahmp_hip_debug_copy_stats counts both kinds."""
    import ctypes as C
    import torch
    s = synth.mixed_small(tables[1], ni=1024, nj=640, seed=37)              # 2.6 MB per 2-D array, 18 MB for ZSNSOXY
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 13, t_offset=s.t_offset)
    d = s.to_device("cuda:0")
    engine.noahmplsm(d, 1, 2000, 180.0)
    want = d.to_host()

    def stats():
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        engine.lib.noahmp_hip_debug_copy_stats(C.byref(a), C.byref(b))
        return a.value, b.value
    up = sum(v.nbytes for k, v in s.a.items() if k != "dzs")
    down = sum(v.nbytes for k, v in s.a.items() if k != "dzs" and FIELD_INFO[k][2] != "in")
    prev = engine.set_option("host_chunks", 0)
    try:
        h = s.copy()                                                        # plain numpy arrays: pageable
        s0, d0 = stats()
        engine.noahmplsm(h, 1, 2000, 180.0)
        s1, d1 = stats()
        assert (s1 - s0, d1 - d0) == (up + down, 0)
        for k in _outs(h):
            np.testing.assert_array_equal(h.a[k], want.a[k], err_msg=k)
        p = s.copy()                                                        # the same arrays in page-locked memory (torch's allocator)
        keep = {}
        for k, v in p.a.items():
            if k != "dzs":
                keep[k] = torch.empty(v.shape, dtype=torch.from_numpy(v).dtype, pin_memory=True)
                keep[k].numpy()[...] = v
                p.a[k] = keep[k].numpy()
        engine.noahmplsm(p, 1, 2000, 180.0)
        s2, d2 = stats()
        assert (s2 - s1, d2 - d1) == (0, up + down)
        for k in _outs(p):
            np.testing.assert_array_equal(p.a[k], want.a[k], err_msg=k)
    finally:
        engine.set_option("host_chunks", prev)


def test_pipelined_host_path_bit_identical(engine, tables):
    """Large tiles on the host-memory path are advanced in row chunks (H2D | kernel | D2H on three streams): same bits as
    the device-resident path, untouched cells preserved, fatal column reported with its index in the whole tile."""
    from noahmp_amd.driver import NoahMPFatal
    s = synth.mixed_small(tables[1], ni=512, nj=96, seed=13)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 13, t_offset=s.t_offset)
    r = np.random.default_rng(3)
    s["xland"][r.random(size=(96, 512)) < 0.05] = 2.0            # open water: every output must come back as it went in
    for k in ("hfx", "t2mvxy", "chb2xy", "bgapxy"):
        s.a[k][...] = r.normal(size=s.a[k].shape).astype(np.float32)
    h, d = s.copy(), s.to_device("cuda:0")
    prev = {k: engine.set_option(k, v) for k, v in (("host_chunks", 6), ("pin_host_arrays", 1), ("trust_out_mirror", 0))}
    try:
        for it in (1, 2, 3):                                       # 2nd call pins the arrays, 3rd runs pinned
            sh = engine.noahmplsm(h, it, 2000, 180.0)
            sd = engine.noahmplsm(d, it, 2000, 180.0)
            assert (sh.n_land, sh.n_glacier, sh.n_skipped) == (sd.n_land, sd.n_glacier, sd.n_skipped) and sh.n_skipped > 0
            dh = d.to_host()
            for k in _outs(h):
                np.testing.assert_array_equal(h.a[k], dh.a[k], err_msg="%s step %d" % (k, it))
        water = s["xland"] > 1.5
        for k in ("hfx", "t2mvxy", "chb2xy", "bgapxy"):
            np.testing.assert_array_equal(h.a[k][water], s.a[k][water], err_msg=k)
        bad = s.copy()
        bad["isltyp"][70, 300] = 25                               # a row that lives in a late chunk
        bad["isltyp"][80, 5] = 25
        with pytest.raises(NoahMPFatal) as e:
            engine.noahmplsm(bad, 1, 2000, 180.0)
        assert (e.value.code, e.value.i, e.value.j) == (1, 301, 71)
        engine.set_option("trust_out_mirror", 1)                   # OUT arrays not re-uploaded after the first call
        t1, t2 = s.copy(), s.copy()
        engine.set_option("host_chunks", 0)
        engine.noahmplsm(t1, 1, 2000, 180.0); engine.noahmplsm(t1, 2, 2000, 180.0)
        engine.set_option("host_chunks", 6)
        engine.noahmplsm(t2, 1, 2000, 180.0); engine.noahmplsm(t2, 2, 2000, 180.0)
        for k in _outs(t1):
            np.testing.assert_array_equal(t1.a[k], t2.a[k], err_msg=k)
    finally:
        for k, v in prev.items():
            engine.set_option(k, v)


def test_resident_host_path_lazy_download(engine, port, tables):
    """Host arrays, state resident in the device mirrors ("resident_state" + "lazy_download"): per call only the IN arrays
    travel; the results appear in the host arrays at noahmp_hip_fetch -- and are the bits of the ordinary host path."""
    s = synth.mixed_small(tables[1], ni=128, nj=8, seed=23)
    synth.first_step_fixups(s)
    plain, res = s.copy(), s.copy()
    start = res.copy()
    nsteps = 12
    for it in range(1, nsteps + 1):
        synth.diurnal_forcing(plain, (it - 1) % 24, t_offset=s.t_offset)
        engine.noahmplsm(plain, it, 2000, 180.0)
    try:
        engine.set_option("resident_state", 1)
        engine.set_option("lazy_download", 1)
        for it in range(1, nsteps + 1):
            synth.diurnal_forcing(res, (it - 1) % 24, t_offset=s.t_offset)       # in place: same arrays every call
            st = engine.noahmplsm(res, it, 2000, 180.0)
            assert st.code == 0 and st.n_land > 0
        np.testing.assert_array_equal(res["tslb"], start["tslb"])                  # nothing came back yet
        np.testing.assert_array_equal(res["hfx"], start["hfx"])
        engine.fetch()
        _check(plain, res, engine, steps=nsteps, fields=_outs(plain))
        # another set of arrays: the engine notices, uploads everything and keeps going
        other = plain.copy()
        synth.diurnal_forcing(other, nsteps % 24, t_offset=s.t_offset)
        synth.diurnal_forcing(plain, nsteps % 24, t_offset=s.t_offset)
        engine.noahmplsm(other, nsteps + 1, 2000, 180.0)
        engine.fetch()
    finally:
        engine.set_option("lazy_download", 0)
        engine.set_option("resident_state", 0)
    engine.noahmplsm(plain, nsteps + 1, 2000, 180.0)
    _check(plain, other, engine, steps=nsteps + 1, fields=_outs(plain))


def test_resident_host_path_static_inputs_and_deferred_status(engine, tables):
    """"static_inputs" + "deferred_status" on top of resident_state + lazy_download: 12 steps give the bits of the ordinary host path;
    a call reports the PREVIOUS step (tallies, fatal column), the last step's fatal comes out of fetch; a static array changed
    behind the engine's back is (by contract) not seen until the state is rebuilt."""
    from noahmp_amd.driver import NoahMPFatal
    s = synth.mixed_small(tables[1], ni=128, nj=8, seed=67)
    synth.first_step_fixups(s)
    plain, res = s.copy(), s.copy()
    nsteps = 12
    tallies = []
    for it in range(1, nsteps + 1):
        synth.diurnal_forcing(plain, (it - 1) % 24, t_offset=s.t_offset)
        st = engine.noahmplsm(plain, it, 2000, 180.0)
        tallies.append((st.n_land, st.n_glacier, st.n_skipped))
    try:
        for k, v in (("resident_state", 1), ("lazy_download", 1), ("static_inputs", 1), ("deferred_status", 1)):
            engine.set_option(k, v)
        for it in range(1, nsteps + 1):
            synth.diurnal_forcing(res, (it - 1) % 24, t_offset=s.t_offset)      # in place: same arrays every call
            st = engine.noahmplsm(res, it, 2000, 180.0)
            assert st.code == 0
            assert (st.n_land, st.n_glacier, st.n_skipped) == ((0, 0, 0) if it == 1 else tallies[it - 2])      # the previous step's
            res["coszin"][...] = -5.0                                           # the caller may overwrite its forcing right away
        engine.fetch()
        _check(plain, res, engine, steps=nsteps, fields=_outs(plain))
        # a fatal column (soil type out of range) in the LAST step: the call itself returns 0, fetch reports it
        bad = res.copy()
        synth.diurnal_forcing(bad, 3, t_offset=s.t_offset)
        engine.set_option("static_inputs", 0)                                   # ISLTYP is a static array: let the change through
        bad["isltyp"][2, 5] = 99
        st = engine.noahmplsm(bad, nsteps + 1, 2000, 180.0, check=False)
        assert st.code == 0
        rc = engine.lib.noahmp_hip_fetch(None)
        assert rc == 1, rc                                                      # NOAHMP_ERR_SOILTYP_RANGE
    finally:
        for k in ("deferred_status", "static_inputs", "lazy_download", "resident_state"):
            engine.set_option(k, 0)


@pytest.mark.parametrize("deferred", [0, 1], ids=["sync", "deferred"])
def test_resident_host_path_sorted_mirrors(engine, tables, deferred):
    """"resident_sorted" (+ resident_state, lazy_download, static_inputs): the state additionally lives in device mirrors sorted by (class,
    vegetation type, snow-layer count, TSK bin) and the class-range kernels run on them -- host arrays in tile order in, the bits of the
    ordinary host path out: over 30 steps (the state is sorted again after 24), with a fetch in the middle, with open water, sea ice and
    land ice in the tile, with and without deferred status; a fatal column is reported at its TILE position."""
    from noahmp_amd.driver import NoahMPFatal
    s = synth.mixed_small(tables[1], ni=192, nj=24, glacier_frac=0.06, seed=77)
    r = np.random.default_rng(5)
    s["xland"][r.random(size=(24, 192)) < 0.04] = 2.0
    s["xice"][3, 10:17] = 1.0
    synth.first_step_fixups(s)
    plain, res = s.copy(), s.copy()
    nsteps = 30
    for it in range(1, nsteps + 1):
        synth.diurnal_forcing(plain, (it + 5) % 24, t_offset=s.t_offset)
        engine.noahmplsm(plain, it, 2000, 180.0)
        if it == 10:
            mid = plain.copy()
    opts = (("resident_state", 1), ("lazy_download", 1), ("static_inputs", 1), ("resident_sorted", 1), ("deferred_status", deferred))
    try:
        for k, v in opts:
            engine.set_option(k, v)
        kernel_ms = []
        for it in range(1, nsteps + 1):
            synth.diurnal_forcing(res, (it + 5) % 24, t_offset=s.t_offset)
            st = engine.noahmplsm(res, it, 2000, 180.0)
            assert st.code == 0
            kernel_ms.append(st.kernel_ms)
            if it == 10:
                engine.fetch()
                _check(mid, res, engine, steps=10, fields=_outs(plain))
        engine.fetch()
        _check(plain, res, engine, steps=nsteps, fields=_outs(plain))
        # a fatal column: reported at its (i, j) of the TILE although the kernel saw it at a sorted position
        bad = res.copy()
        synth.diurnal_forcing(bad, 14, t_offset=s.t_offset)
        bad["isltyp"][17, 101] = 99                         # other arrays: the state is rebuilt and sorted again, the soil type is seen
        st = engine.noahmplsm(bad, nsteps + 1, 2000, 180.0, check=False)
        rc = engine.lib.noahmp_hip_fetch(None) if deferred else st.code
        assert rc == 1, rc                                  # NOAHMP_ERR_SOILTYP_RANGE
        if not deferred:
            assert (st.i, st.j) == (102, 18), (st.code, st.i, st.j)
    finally:
        for k, _ in reversed(opts):
            engine.set_option(k, 0)


@pytest.mark.parametrize("event", ["static_inputs_off_on", "sub_tile_call"])
def test_resident_sorted_set_is_dropped_when_it_cannot_serve_a_call(engine, tables, event):
    """The sorted mirror set of "resident_sorted" must never be used stale (round 5's advisor finding): while it holds the newest state,
    (a) the caller withdraws and re-declares "static_inputs" (and changes a vegetation type in between), or (b) advances a SUB-tile of
    the same arrays (its > ims: the sorted set cannot serve it) -- the kernels then run on the tile-order mirrors, which must have been
    brought up to date first, and a later full-tile call must sort the state anew.  Bits of the ordinary host path throughout."""
    s = synth.mixed_small(tables[1], ni=160, nj=16, glacier_frac=0.05, seed=91)
    synth.first_step_fixups(s)
    plain, res = s.copy(), s.copy()

    def forcing(st, it):
        synth.diurnal_forcing(st, (it + 7) % 24, t_offset=s.t_offset)

    def both(it, **idx):
        for st in (plain, res):
            forcing(st, it)
            if idx:
                st.set_index(**idx)
        for k in ("resident_state", "lazy_download", "static_inputs", "resident_sorted"):
            prev[k] = engine.set_option(k, 0)                                   # the plain path for `plain` ...
        engine.noahmplsm(plain, it, 2000, 180.0)
        for k in ("resident_state", "lazy_download", "static_inputs", "resident_sorted"):
            engine.set_option(k, prev[k])                                       # ... and whatever the test has switched on for `res`
        assert engine.noahmplsm(res, it, 2000, 180.0).code == 0
    prev = {}
    opts = ("resident_state", "lazy_download", "static_inputs", "resident_sorted")
    try:
        for k in opts:
            engine.set_option(k, 1)
        for it in (1, 2, 3):
            both(it)                                                            # the sorted set now holds the newest state
        if event == "static_inputs_off_on":
            engine.set_option("static_inputs", 0)                              # fetches; both mirror sets will be rebuilt
            for st in (plain, res):
                st["ivgtyp"][5, 40:60] = 14                                    # the caller MAY change static inputs now
            both(4)
            both(5)
            engine.set_option("static_inputs", 1)
            both(6)
            both(7)
        else:
            full = dict(its=1, ite=160, jts=1, jte=16)
            both(4, its=9, ite=150, jts=3, jte=14)                              # a sub-tile of the same arrays: tile-order kernel
            both(5, its=9, ite=150, jts=3, jte=14)
            both(6, **full)                                                     # full tile again: sorted anew
            both(7, **full)
        engine.fetch()
        _check(plain, res, engine, steps=7, fields=_outs(plain))
    finally:
        for k in reversed(opts):
            engine.set_option(k, 0)


def test_resident_host_path_alternating_tiles_of_different_size(engine, tables):
    """Two tiles (nests) of different extents advanced alternately with "resident_state" + "lazy_download": a call with other
    arrays first brings the previous tile's host arrays up to date from the still intact mirrors, and only then re-sizes the
    mirrors -- every tile ends with the bits of the ordinary host path."""
    big = synth.mixed_small(tables[1], ni=160, nj=12, seed=61)
    small = synth.mixed_small(tables[1], ni=48, nj=5, seed=62)
    for s in (big, small):
        synth.first_step_fixups(s)
    want = {}
    for name, s in (("big", big), ("small", small)):
        p = s.copy()
        for it in (1, 2):
            synth.diurnal_forcing(p, 11 + it, t_offset=s.t_offset)
            engine.noahmplsm(p, it, 2000, 180.0)
        want[name] = p
    try:
        engine.set_option("resident_state", 1)
        engine.set_option("lazy_download", 1)
        for it in (1, 2):
            for s in (big, small):                       # big, small, big, small: every call meets the other tile's mirrors
                synth.diurnal_forcing(s, 11 + it, t_offset=s.t_offset)
                assert engine.noahmplsm(s, it, 2000, 180.0).code == 0
        engine.fetch()
    finally:
        engine.set_option("lazy_download", 0)
        engine.set_option("resident_state", 0)
    _check(want["big"], big, engine, steps=2, fields=_outs(big))
    _check(want["small"], small, engine, steps=2, fields=_outs(small))


@pytest.mark.parametrize("dveg,run", [(1, 1), (3, 1), (4, 1), (4, 3), (2, 1)])
def test_option_specialised_kernels_bit_identical(engine, tables, dveg, run):
    """Calls whose options are the reference's namelist values (DVEG 1 or 3) run kernels compiled with those options as
    constants (noahmp_engine_dveg*.hip); they must return the bits of the generic kernel -- mixed tile and class ranges alike.
    (DVEG 2, RUN 1) has no specialised kernel: both settings run the generic one."""
    cfg = ModelConfig(idveg=dveg, iopt_run=run)
    s = synth.mixed_small(tables[1], ni=128, nj=12, glacier_frac=0.06, seed=53, cfg=cfg)
    synth.first_step_fixups(s)
    res = {}
    for fixed in (1, 0):
        engine.set_option("fixed_option_kernels", fixed)
        try:
            tile, srt = s.to_device("cuda:0"), s.to_device("cuda:0")
            perm = engine.sort_store(srt).cpu().numpy()
            for it in range(1, 7):
                synth.diurnal_forcing(s, (it + 9) % 24, t_offset=s.t_offset)
                import torch
                for k in ("coszin", "swdown", "glw", "t3d", "rainbl"):
                    v = torch.from_numpy(s.a[k]).cuda()
                    tile.a[k].copy_(v)
                    srt.a[k].copy_((v.permute(0, 2, 1).reshape(-1, v.shape[1])[torch.from_numpy(perm).long().cuda()]
                                    .reshape(v.shape[0], v.shape[2], v.shape[1]).permute(0, 2, 1)) if v.dim() == 3
                                   else v.reshape(-1)[torch.from_numpy(perm).long().cuda()].reshape(v.shape))
                assert engine.noahmplsm(tile, it, 2000, 180.0).code == 0
                assert engine.noahmplsm(srt, it, 2000, 180.0).code == 0
            res[fixed] = (tile.to_host(), srt.to_host())
        finally:
            engine.set_option("fixed_option_kernels", 1)
    for which in (0, 1):
        _check(res[0][which], res[1][which], engine, steps=6, fields=_outs(res[0][which]))
    a, b = res[1]
    for k in _outs(a):                                   # and the sorted run is the tile-order run, permuted
        x, y = a.a[k], b.a[k]
        x = x.transpose(0, 2, 1).reshape(-1, x.shape[1])[perm] if x.ndim == 3 else x.reshape(-1)[perm]
        y = y.transpose(0, 2, 1).reshape(-1, y.shape[1]) if y.ndim == 3 else y.reshape(-1)
        assert np.array_equal(x, y, equal_nan=True), k


@pytest.mark.parametrize("kw", [dict(idveg=2, iopt_run=3, iopt_stc=2, iopt_frz=2), dict(iopt_btr=2, iopt_crs=2, idveg=5)],
                         ids=["dveg2_run3_stc2_frz2", "btr2_crs2_dveg5"])
def test_runtime_compiled_kernels_bit_identical(engine, tables, kw):
    """Option sets without an ahead-of-time specialised kernel: by default ("jit_option_kernels" = 1) the engine compiles one at the
    first call (hiprtc, or loads it from the on-disk cache) -- it must return the bits of the generic kernel, mixed tile and class
    ranges alike."""
    import torch
    cfg = ModelConfig(**kw)
    s = synth.mixed_small(tables[1], ni=128, nj=12, glacier_frac=0.06, seed=59, cfg=cfg)
    synth.first_step_fixups(s)
    synth.diurnal_forcing(s, 13, t_offset=s.t_offset)
    res = {}
    assert engine.set_option("jit_option_kernels", -1) == 1          # the default (reading: an invalid value changes nothing)
    for jit in (0, 1):
        engine.set_option("jit_option_kernels", jit)
        try:
            tile, srt = s.to_device("cuda:0"), s.to_device("cuda:0")
            engine.sort_store(srt, tsk_bin=0)
            for it in range(1, 5):
                assert engine.noahmplsm(tile, it, 2000, 180.0).code == 0
                assert engine.noahmplsm(srt, it, 2000, 180.0).code == 0
            res[jit] = (tile.to_host(), srt.to_host())
            if jit:
                msg = engine.lib.noahmp_hip_last_error().decode()
                assert "generic kernel used" not in msg, msg          # the run-time compiled kernels really ran
                d, compiled, hits, fallbacks = engine.jit_cache_info()
                assert d and compiled + hits >= 1 and fallbacks == 0, (d, compiled, hits, fallbacks)
        finally:
            engine.set_option("jit_option_kernels", 1)
    for which in (0, 1):
        _check(res[0][which], res[1][which], engine, steps=4, fields=_outs(res[0][which]))
