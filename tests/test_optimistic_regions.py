"""The optimistic regions of the option-specialised land kernels (VEGE_FLUX's loop1, BARE_FLUX's loop3, SOILWATER): a pass with the unchecked libm forms,
redone per wave with the checked forms when a lane met a rare argument.  The results must be the bits of the all-checked code in every
case: the redo is invisible.

CPU: the host emulation of the device source compiled twice, with the regions (-DNMP_OPTIMISTIC_REGIONS=1) and all-checked (the default
of the generic source), on the golden mixed tile with a NaN, a zero and a 1e38 planted in SMC, SFCTMP and SOLDN (and TG, TV, which reach loop1) of a few columns: on
the host every column decides for itself, so planted columns take the redo and the others do not; a counter per region shows that each did.
GPU: (i) "force_checked_regions" = 1 (every wave takes the redo) against the default on the full-size config-3 grid (whole arrays), the
config-5 full-size sample and the option fuzz; (ii) the planted tile through the specialised kernels against the generic kernel, status
words included.  Every comparison is bit for bit, allow_cols = 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, load_store
from noahmp_amd import synth
from noahmp_amd.abi import FIELD_INFO
from noahmp_amd.state import ModelConfig

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _outs(store):
    return [k for k in store.a if FIELD_INFO[k][2] != "in"]


def _assert_stores_bit_equal(a, b, what):
    for k in _outs(a):
        x, y = a.a[k], b.a[k]
        assert np.array_equal(x, y, equal_nan=True), "%s differs (%s): %d elements" % (k, what, int((~((x == y) | ((x != x) & (y != y)))).sum()))


PLANTS = (np.float32("nan"), np.float32(0.0), np.float32(1e38))


def plant_state(s):
    """A NaN, a zero and a 1e38 in SMC (all layers and the top layer alone) of a few columns, and in TG and TV of others: SMC reaches
    SOILWATER's powers, and a 1e38 ground or leaf temperature overflows the heat fluxes of VEGE_FLUX's loop1, whose Monin-Obukhov lengths
    then send inf into SFCDIF1's and RAGRB's powers.  Arrays are (j, k, i)."""
    sm = s.a["smois"]
    nj, ni = sm.shape[0], sm.shape[2]
    n = 0
    for v in PLANTS:
        for whole in (True, False):
            i, j = (7 + 5 * n) % ni, n % nj
            if whole:
                sm[j, :, i] = v
            else:
                sm[j, 0, i] = v
            n += 1
    for key in ("tgxy", "tvxy"):
        for v in PLANTS:
            for rep in range(6):                   # several columns each: only those with a canopy run loop1
                i, j = (3 + 7 * n) % ni, n % nj
                s.a[key][j, i] = v
                n += 1


def plant_forcing(s):
    """the same three values in SFCTMP (T3D, lowest level) and SOLDN (SWDOWN) of other columns; after every forcing update"""
    t3d, sw = s.a["t3d"], s.a["swdown"]
    nj, ni = sw.shape
    n = 0
    for v in PLANTS:
        i, j = (11 + 3 * n) % ni, (n + 1) % nj
        t3d[j, 0, i] = v
        i, j = (19 + 7 * n) % ni, (n + 2) % nj
        sw[j, i] = v
        n += 1


def golden_planted():
    g = np.load(os.path.join(GOLDEN, "golden_mixed.npz"))
    s = load_store(g, "init", 64, 4)
    plant_state(s)
    return s, g["t_offset"]


# ---- CPU: host emulation, regions on against all-checked ---------------------------------------------------------------------------------
EMUL_VARIANTS = {"checked": ("-DNMP_OPTIMISTIC_REGIONS=0", "libnmp_emul_checked.so"), "optimistic": ("-DNMP_OPTIMISTIC_REGIONS=1 -DNMP_REGION_COUNT", "libnmp_emul_optimistic.so")}


def build():
    """the two host-emulation libraries (all-checked, regions on); returns their paths"""
    csrc = os.path.join(ROOT, "noahmp_amd", "csrc")
    src = os.path.join(HERE, "host_emul", "emul.hip")
    deps = [src, os.path.join(ROOT, "include", "noahmp_hip.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    out = {}
    for key, (flag, name) in EMUL_VARIANTS.items():
        lib = out[key] = os.path.join(HERE, "host_emul", name)
        if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                                   "-mfma", "-Wno-unused-value", "-DNOAHMP_NSOIL=4"] + flag.split() + ["-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                                   src, "-o", lib])
    return out


def _emul_variant(tables, lib):
    import tests.host_emul.emullib as m
    old = m.build
    m.build = lambda nsoil=4: lib
    try:
        e = m.EmulLib()
    finally:
        m.build = old
    e.set_tables(tables[0])
    return e


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
@pytest.mark.parametrize("kw", [dict(), dict(iopt_run=5, idveg=3), dict(iopt_run=2), dict(iopt_run=3, iopt_inf=2, iopt_sfc=2), dict(iopt_run=4)],
                         ids=lambda k: repr(k))
def test_host_emulation_regions_equal_all_checked(tables, kw):
    libs = build()
    checked, optimistic = _emul_variant(tables, libs["checked"]), _emul_variant(tables, libs["optimistic"])
    s, toff = golden_planted()
    s.cfg = ModelConfig(**kw) if kw else s.cfg
    a, b = s.copy(), s.copy()
    redos = (C.c_long * 3).in_dll(optimistic.lib, "nmp_region_redos")      # VEGE_FLUX loop1, BARE_FLUX loop3, SOILWATER (-DNMP_REGION_COUNT)
    redos[0] = redos[1] = redos[2] = 0
    for it in range(1, 7):
        for x in (a, b):
            synth.diurnal_forcing(x, (it + 8) % 24, t_offset=toff)
            plant_forcing(x)
        sa = checked.noahmplsm(a, it, 2000, 180.0)
        sb = optimistic.noahmplsm(b, it, 2000, 180.0)
        assert (sa.code, sa.n_land, sa.n_glacier) == (sb.code, sb.n_land, sb.n_glacier), it
        _assert_stores_bit_equal(a, b, "step %d %r" % (it, kw))
    n_steps_cols = 6 * a.a["tgxy"].size
    print("redos (loop1, loop3, soilwater):", list(redos), "of", n_steps_cols, "column-steps")
    # every wrapper was driven into its redo by a planted column, and the unplanted columns (the great majority) were not
    want = [0, 1, 2] if kw.get("iopt_sfc", 1) == 1 else [0, 2]      # under OPT_SFC = 2 loop3 has SFCDIF2 only, which keeps the checked forms
    assert all(0 < redos[r] < n_steps_cols // 2 for r in want), list(redos)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def forced(engine):
    """every wave of an optimistic region takes the checked redo"""
    assert engine.set_option("force_checked_regions", 1) == 0
    yield engine
    engine.set_option("force_checked_regions", 0)


@pytest.mark.gpu
def test_gpu_force_checked_config3_full_size_bit_identical(engine, tables):
    """BASELINE configs[2] at its full size (4608 x 1536 columns, the grid bench.py times), 12 hourly steps on the device-sorted layout,
    default against "force_checked_regions" = 1: every INOUT / OUT array whole, bit for bit."""
    import torch
    from test_sort_gpu import FKEYS
    gx, gy = 4608, 1536
    s = synth.config3_tile(tables[1], gx, gy, cfg=ModelConfig())
    synth.first_step_fixups(s)
    forc = {}
    state = {k: s.a[k].copy() for k in s.a}
    for h in range(12):
        synth.diurnal_forcing(s, (h + 6) % 24, t_offset=s.t_offset)
        forc[h] = {k: torch.from_numpy(s.a[k].copy()).cuda() for k in FKEYS}
    for k in state:
        s.a[k][...] = state[k]
    res = {}
    for force in (0, 1):
        assert engine.set_option("force_checked_regions", force) in (0, 1)
        try:
            d = s.to_device("cuda:0")
            perm = engine.sort_store(d)
            sc = engine.scatter([d.a[k] for k in FKEYS], [forc[0][k] for k in FKEYS], perm, gx, gy)
            args = d.step_args(1, 2000, 180.0)
            for it in range(1, 13):
                sc.set_sources([forc[it - 1][k] for k in FKEYS])
                sc()
                args.itimestep = it
                engine.noahmplsm_async(args)
            st, _ = engine.sync()
            assert st.code == 0
            res[force] = d
        finally:
            engine.set_option("force_checked_regions", 0)
    for k in _outs(s):
        x, y = res[0].a[k], res[1].a[k]
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), k


@pytest.mark.gpu
def test_gpu_force_checked_config5_full_size_sample_bit_identical(forced):
    """BASELINE configs[4] at its full size with every wave taking the redo: the sample is the oracle's, bit for bit, as the default's is
    (tests/test_config5.py::test_gpu_config5_full_size_sample_bit_identical)"""
    from tools.config5_run import run
    res = run(3600, 1800, nsteps=12, nsample=4096, verbose=False, checkpoints=(1,))
    assert res["device_status_max"] == 0, res
    assert res["sample_bit_identical"], res


@pytest.mark.gpu
def test_gpu_force_checked_option_fuzz_bit_identical(forced, port):
    """the option fuzz of tests/test_fuzz.py (ahead-of-time and run-time specialised kernels) with every wave taking the redo: the oracle's
    bits, as the default's are"""
    from tools import fuzz_parity
    from test_fuzz import OPTS, SCALARS
    for kw in OPTS:
        assert fuzz_parity.one_seed("gpu", 303, 4096, kw) == 0, kw
    for kw in SCALARS:
        assert fuzz_parity.one_seed("gpu", 14, 4096, kw) == 0, kw
    assert fuzz_parity.one_seed("gpu", 3, 4096, dict(nan=1, scalars=1)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(idveg=3, iopt_run=5), dict(idveg=4, iopt_run=3), dict(idveg=2, iopt_run=2, iopt_sfc=2),
                                dict(iopt_run=4, iopt_inf=2)], ids=lambda k: repr(k))
def test_gpu_planted_specials_specialised_equals_generic(engine, tables, kw):
    """the golden mixed tile with a NaN, a zero and a 1e38 planted in SMC, SFCTMP and SOLDN of a few columns: the specialised kernels
    (ahead of time or compiled at run time; waves with a planted column take the redo, the others do not) against the generic kernel,
    which has the checked forms only.  Outputs and status words, bit for bit."""
    from noahmp_amd.driver import NoahMPFatal
    s, toff = golden_planted()
    if kw:
        s.cfg = ModelConfig(**kw)
    res = {}
    for fixed in (1, 0):
        engine.set_option("fixed_option_kernels", fixed)
        engine.set_option("jit_option_kernels", fixed)
        try:
            x = s.copy()
            status = []
            for it in range(1, 7):
                synth.diurnal_forcing(x, (it + 8) % 24, t_offset=toff)
                plant_forcing(x)
                try:
                    st = engine.noahmplsm(x, it, 2000, 180.0)      # host-memory path
                    status.append((st.code, st.n_land, st.n_glacier))
                except NoahMPFatal as e:                           # a planted column may be fatal: then it is the same column with the same code
                    status.append((e.code, e.i, e.j))
            res[fixed] = (x, status)
        finally:
            engine.set_option("fixed_option_kernels", 1)
            engine.set_option("jit_option_kernels", 1)
    assert res[0][1] == res[1][1], (res[0][1], res[1][1])
    _assert_stores_bit_equal(res[0][0], res[1][0], repr(kw))
