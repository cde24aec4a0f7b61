"""Device-side history: interval accumulators and point probes (noahmp_hip_history_step / noahmp_hip_history_finish,
noahmp_amd/csrc/noahmp_history.hip, noahmp_amd/history.py).

Every comparison is a BIT comparison (the conventions of tools/compare.py::exact_check: NaN equals NaN, no element may differ): the
feature has no tolerance.  CPU: the per-element functions of nmp_dev_history.hpp compiled for the host (tests/host_emul/history_check.hip,
built on demand) against the reference's own accumulators and a numpy restatement; the generated bindings; the output file; the Fortran
driver's build.  GPU: the kernels against the oracle advanced through the same chain."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from noahmp_amd import abi, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "noahmp_amd", "csrc")
SRC = os.path.join(HERE, "host_emul", "history_check.hip")
LIB = os.path.join(HERE, "host_emul", "libhistory_check.so")
GOLDEN = os.path.join(HERE, "golden")
F = np.float32
OPS = ("sum", "sum_dt", "min", "max", "last")
HUGE = np.finfo(np.float32).max


# ---------------------------------------------------------------------------------------------------------------- helpers
def build():
    deps = [SRC, os.path.join(CSRC, "nmp_dev_history.hpp"), os.path.join(ROOT, "include", "noahmp_hip.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
                               "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SRC, "-o", LIB])


def _host():
    build()
    try:
        import torch  # noqa: F401  (map torch's HIP runtime first, noahmp_amd/abi.py::load_library)
    except ImportError:
        pass
    lib = C.CDLL(LIB)
    lib.history_apply.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_long]
    lib.history_takes_part.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_long]
    lib.history_finish.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_long]
    return lib


def host_apply(lib, op, acc, x, scale=0.0, part=None):
    acc = np.ascontiguousarray(acc, dtype=F).copy()
    x = np.ascontiguousarray(x, dtype=F)
    p = None if part is None else np.ascontiguousarray(part, dtype=np.uint8)
    lib.history_apply(abi.HIST_OP[op], acc.ctypes.data, x.ctypes.data, float(scale), p.ctypes.data if p is not None else None, acc.size)
    return acc


def np_apply(op, acc, x, scale=0.0, part=None):
    """The numpy float32 restatement of one sample (float32 arrays: every numpy operation rounds to float32)."""
    acc, x = np.asarray(acc, dtype=F), np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        r = {"sum": lambda: acc + x,
             "sum_dt": lambda: acc + (x * F(scale)),
             "min": lambda: np.where(x < acc, x, acc),
             "max": lambda: np.where(x > acc, x, acc),
             "last": lambda: x}[op]().astype(F)
    return r if part is None else np.where(part, r, acc).astype(F)


def np_takes_part(xland, xice, thres):
    with np.errstate(all="ignore"):
        return ~((xland - F(1.5)) >= 0) & ~(xice >= F(thres))


def np_finish(acc, count, mean, fill):
    if not mean:
        return acc.copy()
    with np.errstate(all="ignore"):
        return np.where(count == 0, F(fill), acc / np.maximum(count, 1).astype(F)).astype(F)


def assert_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    assert a.shape == b.shape, what
    bad = ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], a[tuple(np.argwhere(bad)[0])], b[tuple(np.argwhere(bad)[0])])


def nasty(r, n):
    """Random float32 values that contain NaN, +-Inf, -0.0, zeros and denormals."""
    x = (r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-42, HUGE, -HUGE], dtype=F)
    at = r.random(n) < 0.25
    x[at] = special[r.integers(0, len(special), int(at.sum()))]
    return x


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("acc_name, flux_name", [("udrunoff", "runsbxy"), ("sfcrunoff", "runsfxy")])
def test_sum_dt_reproduces_the_reference_accumulators(acc_name, flux_name):
    """Reference pin: SUM_DT of traj/runsbxy (runsfxy) of golden_config1.npz -- written by the compiled reference -- with scale DT = 3600,
    started from init/udrunoff (sfcrunoff), gives the bits of the reference's own traj/udrunoff (sfcrunoff) at each of the 24 steps
    (drv:733-734, 798-799).  The pair must have non-zero samples: a pin on zeros pins nothing."""
    lib = _host()
    z = np.load(os.path.join(GOLDEN, "golden_config1.npz"))
    nonzero = {}
    for a, f in (("udrunoff", "runsbxy"), ("sfcrunoff", "runsfxy")):
        nonzero[a] = int(np.count_nonzero(z["traj/" + f]))
    assert nonzero["udrunoff"] > 0 or nonzero["sfcrunoff"] > 0, nonzero
    assert nonzero[acc_name] > 0, "no non-zero sample of %s in the fixture" % flux_name
    acc = z["init/" + acc_name].astype(F)
    flux, want = z["traj/" + flux_name], z["traj/" + acc_name]
    assert flux.shape[0] == 24
    for it in range(24):
        acc = host_apply(lib, "sum_dt", acc, flux[it], 3600.0)
        assert_bits(acc, want[it], "%s after step %d" % (acc_name, it + 1))


@pytest.mark.parametrize("op", OPS)
def test_every_op_against_numpy_on_special_values(op):
    lib = _host()
    r = np.random.default_rng(101 + OPS.index(op))
    n = 20000
    acc, part = nasty(r, n), r.random(n) < 0.8
    for k in range(3):
        x = nasty(r, n)
        got = host_apply(lib, op, acc, x, 3600.0, part)
        assert_bits(got, np_apply(op, acc, x, 3600.0, part), "%s sample %d" % (op, k))
        acc = got
    # the special values are really there, on both sides
    assert np.isnan(x).any() and np.isinf(x).any() and (np.signbit(x) & (x == 0)).any() and ((x != 0) & (np.abs(x) < 1e-38)).any()


def test_sum_dt_is_two_roundings_not_a_fused_multiply_add():
    """acc + x * s with the product rounded to float32 first (drv:733-739): on this input set the fused result (exact product, one
    rounding) differs for some samples, so a contracted multiply-add cannot pass."""
    lib = _host()
    r = np.random.default_rng(7)
    n = 50000
    x = r.uniform(1e-7, 3e-4, n).astype(F)                  # runoff / evaporation rates [mm/s]
    acc = r.uniform(0.0, 50.0, n).astype(F)
    s = F(3600.0)
    two = (acc + (x * s)).astype(F)
    fused = (acc.astype(np.float64) + x.astype(np.float64) * np.float64(s)).astype(F)       # exact in float64 (24 + 24 bit product)
    assert (two.view(np.uint32) != fused.view(np.uint32)).sum() > 100
    got = host_apply(lib, "sum_dt", acc, x, float(s))
    assert_bits(got, two, "SUM_DT")


def test_class_test_and_finish_against_numpy():
    lib = _host()
    r = np.random.default_rng(5)
    n = 4096
    xland = r.choice(np.array([1.0, 2.0, 1.5, 1.4999999, np.nan], dtype=F), n)
    xice = r.choice(np.array([0.0, 0.5, 0.49999997, 1.0, np.nan], dtype=F), n)
    out = np.zeros(n, np.uint8)
    lib.history_takes_part(xland.ctypes.data, xice.ctypes.data, 0.5, out.ctypes.data, n)
    assert np.array_equal(out.astype(bool), np_takes_part(xland, xice, 0.5))
    count = r.integers(0, 25, n).astype(np.int32)
    for op in OPS:
        for mean in (0, 1):
            acc = nasty(r, n)
            a2, dst = acc.copy(), np.zeros(n, F)
            lib.history_finish(abi.HIST_OP[op], a2.ctypes.data, count.ctypes.data, mean, 1, -1e20, dst.ctypes.data, n)
            assert_bits(dst, np_finish(acc, count, mean, -1e20), "finish %s mean=%d" % (op, mean))
            ident = {"sum": F(0), "sum_dt": F(0), "min": HUGE, "max": -HUGE}.get(op)
            assert_bits(a2, acc if ident is None else np.full(n, ident, F), "reset %s" % op)


def test_bindings_regenerate_identically():
    """include/noahmp_hip.h, the Fortran interfaces and oracle/ref_harness_gen.f90 are what tools/gen_abi.py makes of abi_spec.py; the
    oracle's generated wrapper is the committed one (nothing of STEP_FIELDS / WTABLE_FIELDS / TABLE_FIELDS / ERROR_CODES moved)."""
    from tools import gen_abi
    for rel, text in (("include/noahmp_hip.h", gen_abi.c_header()), ("oracle/ref_harness_gen.f90", gen_abi.ref_harness()),
                      ("noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90", gen_abi.fortran_shim()),
                      ("tests/fortran/shim_wrap_gen.f90", gen_abi.shim_wrap())):
        assert open(os.path.join(ROOT, rel)).read() == text, rel
    hdr = open(os.path.join(ROOT, "include", "noahmp_hip.h")).read()
    for word in ("noahmp_history_entry", "noahmp_history_probes", "noahmp_hip_history_step(", "noahmp_hip_history_finish(",
                 "NOAHMP_HIST_SUM_DT", "NOAHMP_HIST_FIN_RESET", "#define NOAHMP_HIP_ABI_VERSION 1"):
        assert word in hdr, word
    f90 = open(os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90")).read()
    assert "bind(C, name='noahmp_hip_history_step')" in f90 and "bind(C, name='noahmp_hip_history_finish')" in f90
    if os.path.isdir(os.path.join(ROOT, ".git")):          # a checkout: the oracle's wrapper is unchanged against git
        r = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "oracle/ref_harness_gen.f90"], capture_output=True, text=True)
        assert r.returncode != 0 or r.stdout.strip() == "", r.stdout


def test_ctypes_mirrors_match_the_compiled_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "noahmp_hip.h"\nint main(){'
                   'printf("%zu %zu %zu %zu %zu %zu", sizeof(noahmp_history_entry), sizeof(noahmp_history_probes),'
                   'offsetof(noahmp_history_entry, scale), offsetof(noahmp_history_probes, field), offsetof(noahmp_history_probes, slot),'
                   'sizeof(noahmp_step_args)); return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out == [C.sizeof(abi.HistoryEntry), C.sizeof(abi.HistoryProbes), abi.HistoryEntry.scale.offset, abi.HistoryProbes.field.offset,
                   abi.HistoryProbes.slot.offset, C.sizeof(abi.StepArgs)]


def output_store():
    """The inputs of the output-file test (and of tests/golden/make_history_output.py): a 6 x 3 host tile, seeded values, two water points."""
    from noahmp_amd.state import ColumnStore
    s = ColumnStore(6, 3)
    r = np.random.default_rng(2024)
    for k in sorted(s.a):
        v = s.a[k]
        if k == "dzs":
            continue
        v[...] = r.integers(1, 20, v.shape) if v.dtype.kind == "i" else r.uniform(-5.0, 300.0, v.shape).astype(F)
    s.a["ivgtyp"][0, 1] = s.a["ivgtyp"][2, 4] = s.cfg.iswater
    extra = {"rainrate": r.uniform(0.0, 1e-3, (3, 6)).astype(F)}
    return s, extra


def test_output_file_without_more_is_the_parent_commits_file(tmp_path):
    """restart.write_output without `more` writes, from the same inputs, the file the commit before this feature wrote
    (tests/golden/history_output_parent.nc, made by tests/golden/make_history_output.py with that commit's restart.py), byte for byte;
    with `more` the added variables follow the reference's list and read back."""
    from scipy.io import netcdf_file
    from noahmp_amd import restart
    s, extra = output_store()
    p0 = restart.write_output(str(tmp_path / "plain.nc"), s, "2000-06-28_12:00:00", extra=extra)
    assert open(p0, "rb").read() == open(os.path.join(GOLDEN, "history_output_parent.nc"), "rb").read()
    r = np.random.default_rng(3)
    acc = r.uniform(0, 9, (3, 6)).astype(F)
    lay = r.uniform(0, 1, (3, 4, 6)).astype(F)
    p1 = restart.write_output(str(tmp_path / "more.nc"), s, "2000-06-28_12:00:00", extra=extra,
                              more=[("ACCECAN", acc, None, "mm"), ("SOIL_M_MEAN", lay, "SOIL", "m{3} m{-3}")])
    f, g = netcdf_file(p1, "r", mmap=False), netcdf_file(p0, "r", mmap=False)
    try:
        names = list(f.variables)
        assert names[:-2] == list(g.variables) and names[-2:] == ["ACCECAN", "SOIL_M_MEAN"]
        assert_bits(f.variables["ACCECAN"][0], acc, "ACCECAN")
        assert_bits(f.variables["SOIL_M_MEAN"][0], lay, "SOIL_M_MEAN")
        assert f.variables["ACCECAN"].units == b"mm" and f.variables["SOIL_M_MEAN"].dimensions[2] == "soil_layers_stag"
        for n in g.variables:
            assert np.array_equal(f.variables[n][:], g.variables[n][:]), n
    finally:
        f.close()
        g.close()
    with pytest.raises(AssertionError):
        restart.write_output(str(tmp_path / "dup.nc"), s, "2000-06-28_12:00:00", extra=extra, more=[("HFX", acc, None, "W m{-2}")])


def _needs_flang():
    from tests.fortran import build_history
    return pytest.mark.skipif(not build_history.available(), reason="flang or oracle/_ref modules missing")


@_needs_flang()
def test_fortran_history_driver_compiles_and_links():
    from tests.fortran import build_history
    if not os.path.exists(abi.LIB_PATH):
        from noahmp_amd import build as b
        b.build()
    lib = build_history.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    assert "history_driver_run" in out
    und = subprocess.check_output(["nm", "-D", "--undefined-only", lib]).decode()
    assert "noahmp_hip_history_step" in und and "noahmp_hip_step_async" in und


# ---------------------------------------------------------------------------------------------------------------- GPU
NSTEP, NI, NJ, DT = 24, 64, 4, 3600.0
FKEYS = ("coszin", "swdown", "glw", "t3d", "rainbl")
PROBE_FIELDS = ("hfx", "lh", "t2mvxy", "tgxy", "grdflx")
WATCH = ("runsfxy", "runsbxy", "hfx", "t2mvxy", "smois", "sfcrunoff", "udrunoff") + PROBE_FIELDS
# (name, field, op, mean): what the scenario accumulates besides the two reference accumulators
EXTRA = [("hfx_mean", "hfx", "sum", True), ("hfx_min", "hfx", "min", False), ("hfx_max", "hfx", "max", False), ("hfx_last", "hfx", "last", False),
         ("t2mv_mean", "t2mvxy", "sum", True), ("t2mv_min", "t2mvxy", "min", False), ("t2mv_max", "t2mvxy", "max", False),
         ("t2mv_last", "t2mvxy", "last", False),
         ("smois_mean", "smois", "sum", True), ("smois_min", "smois", "min", False), ("smois_max", "smois", "max", False),
         ("smois_last", "smois", "last", False)]


def _start(tables):
    s = synth.mixed_small(tables[1], ni=NI, nj=NJ)
    r = np.random.default_rng(11)
    cells = r.choice(NI * NJ, 16, replace=False)
    for c in cells[:8]:                                    # open water; half of them also water in the land-use map (the output mask)
        s["xland"][c // NI, c % NI] = 2.0
    for c in cells[:4]:
        s["ivgtyp"][c // NI, c % NI] = s.cfg.iswater
    for c in cells[8:]:
        s["xice"][c // NI, c % NI] = 1.0                   # sea ice
    synth.first_step_fixups(s)
    r2 = np.random.default_rng(12)
    s["sfcrunoff"] = r2.uniform(0.0, 3.0, (NJ, NI)).astype(F)     # accumulators that continue from state, not from zero
    s["udrunoff"] = r2.uniform(0.0, 3.0, (NJ, NI)).astype(F)
    return s, np.sort(cells)


def _forcing(s, it):
    synth.diurnal_forcing(s, (it - 1) % 24, t_offset=s.t_offset)
    return {k: s.a[k].copy() for k in FKEYS}


@pytest.fixture(scope="module")
def oracle_run(port, tables):
    """The C restatement of the reference advanced 24 steps; per-step copies of the watched arrays."""
    s, skipped = _start(tables)
    o = s.copy()
    steps = []
    for it in range(1, NSTEP + 1):
        o.a.update(_forcing(s, it))
        st = port.noahmplsm(o, it, 2000, 180.0)
        assert st.code == 0
        steps.append({k: o.a[k].copy() for k in WATCH})
    part = np_takes_part(s["xland"], s["xice"], s.cfg.xice_thres)
    assert (~part).sum() == 16 and set(np.flatnonzero(~part.ravel())) == set(skipped)
    return dict(start=s, final=o, steps=steps, part=part)


def _probe_points():
    return np.random.default_rng(13).choice(NI * NJ, 37, replace=False).astype(np.int32)


def _engine_run(engine, tables, sorted_layout):
    """The engine advanced through the same chain with a History sample after every step; probes read back after steps 8, 16, 24."""
    import torch
    from noahmp_amd.history import History
    s, _ = _start(tables)
    d = s.to_device("cuda:0")
    perm = engine.sort_store(d, tsk_bin=0) if sorted_layout else None
    first_perm = perm.clone() if sorted_layout else None
    work = {k: d.a[k] for k in FKEYS}
    src0 = {k: torch.from_numpy(s.a[k].copy()).cuda() for k in FKEYS}
    sc = engine.scatter([work[k] for k in FKEYS], [src0[k] for k in FKEYS], perm, NI, NJ) if sorted_layout else None
    h = History(engine, d)
    h.add("sfcrunoff", "runsfxy", "sum_dt", scale=DT, init=d.a["sfcrunoff"])
    h.add("udrunoff", "runsbxy", "sum_dt", scale=DT, init=d.a["udrunoff"])
    for name, field, op, mean in EXTRA:
        h.add(name, field, op, mean=mean)
    h.add_probes(_probe_points(), PROBE_FIELDS, nslot=8)
    series = []
    for it in range(1, NSTEP + 1):
        f = _forcing(s, it)
        if sorted_layout:
            if it == NSTEP // 2 + 1:                       # one re-sort in the middle, other keys: the History helper follows
                perm = engine.sort_store(d)
                work = {k: d.a[k] for k in FKEYS}
                sc.set_dests([work[k] for k in FKEYS])
                sc.set_perm(perm)
                h.follow(d)
            dev = [torch.from_numpy(f[k]).cuda() for k in FKEYS]
            torch.cuda.synchronize()
            sc.set_sources(dev)
            sc()
        else:
            for k in FKEYS:
                d.a[k].copy_(torch.from_numpy(f[k]))
            torch.cuda.synchronize()
        st = engine.noahmplsm(d, it, 2000, 180.0)
        assert st.code == 0
        h.step()
        if it % 8 == 0:
            series.append(h.read_probes())
    engine.stream_sync()
    count = h.count.clone()
    inv = h._inverse(h.perm) if h.perm is not None else None
    torch.cuda.synchronize()
    raw = {}                                               # the two reference accumulators as they are, brought to tile order by hand
    for it in h.items[:2]:
        flat = it[4].cpu().numpy().ravel()
        raw[it[0]] = (flat[inv.cpu().numpy()] if inv is not None else flat).reshape(NJ, NI)
    out = {k: v.cpu().numpy() for k, v in h.finish().items()}
    cnt_tile = count.cpu().numpy().ravel()
    if inv is not None:
        cnt_tile = cnt_tile[inv.cpu().numpy()]
    after = {it[0]: it[4].cpu().numpy() for it in h.items}
    return dict(out=out, raw=raw, count=cnt_tile.reshape(NJ, NI), count_after=h.count.cpu().numpy(), series=np.concatenate(series), after=after,
                resorted=sorted_layout and not torch.equal(perm, first_perm))


@pytest.fixture(scope="module")
def tile_run(engine, tables):
    return _engine_run(engine, tables, False)


@pytest.fixture(scope="module")
def sorted_run(engine, tables):
    return _engine_run(engine, tables, True)


def _masked(plane, start):
    """What noahmp_hip_history_finish does to a finished plane on water points (netcdf_io:1971-1975)."""
    water = start["ivgtyp"] == start.cfg.iswater
    out = plane.copy()
    out[np.broadcast_to(water[:, None, :] if out.ndim == 3 else water, out.shape)] = F(-1e33)
    return out


@pytest.mark.gpu
def test_runoff_accumulators_are_the_oracles_own(oracle_run, tile_run):
    """SUM_DT(runsfxy, DT) from the initial SFCRUNOFF == the oracle's SFCRUNOFF on every column after 24 steps (skipped columns keep their
    initial bits); likewise UDRUNOFF; count is 24 on advanced columns and 0 on the 16 others."""
    o, part = oracle_run, oracle_run["part"]
    for name in ("sfcrunoff", "udrunoff"):
        assert_bits(tile_run["raw"][name], o["final"][name], name + " (the accumulator plane, every column)")
        assert_bits(tile_run["out"][name], _masked(o["final"][name], o["start"]), name + " (finished: water mask applied)")
        assert_bits(o["final"][name][~part], o["start"][name][~part], name + " of skipped columns")
    assert np.count_nonzero(o["final"]["udrunoff"] != o["start"]["udrunoff"]) > 100
    assert np.array_equal(tile_run["count"], np.where(part, NSTEP, 0))
    assert not tile_run["count_after"].any()               # History.finish(reset=True) starts the next interval


@pytest.mark.gpu
def test_tile_order_and_sorted_layout_agree_and_equal_numpy(oracle_run, tile_run, sorted_run):
    """The same run in tile order and in the sorted layout (one re-sort in the middle that History.follow tracks): finished planes
    identical, and MEAN / MIN / MAX / LAST of hfx, t2mvxy and the 4-level smois equal the numpy restatement applied to the oracle run's
    per-step arrays, the water mask applied."""
    o, part = oracle_run, oracle_run["part"]
    assert sorted_run["resorted"]
    assert set(tile_run["out"]) == set(sorted_run["out"])
    for k in tile_run["out"]:
        assert_bits(tile_run["out"][k], sorted_run["out"][k], "tile order vs sorted layout: " + k)
    for k in tile_run["raw"]:
        assert_bits(sorted_run["raw"][k], o["final"][k], k + " in the sorted layout (every column)")
    assert np.array_equal(tile_run["count"], sorted_run["count"])
    count = np.where(part, NSTEP, 0).astype(np.int32)
    for name, field, op, mean in EXTRA:
        x0 = o["steps"][0][field]
        p = np.broadcast_to(part[:, None, :] if x0.ndim == 3 else part, x0.shape)
        c = np.broadcast_to(count[:, None, :] if x0.ndim == 3 else count, x0.shape)
        acc = np.full(x0.shape, {"sum": 0.0, "min": HUGE, "max": -HUGE, "last": 0.0}[op], F)
        for it in range(NSTEP):
            acc = np_apply(op, acc, o["steps"][it][field], 0.0, p)
        want = _masked(np_finish(acc, c, mean, -1e20), o["start"])
        assert_bits(tile_run["out"][name], want, name)
        ident = {"sum": F(0), "min": HUGE, "max": -HUGE}.get(op)
        if ident is not None:
            assert_bits(tile_run["after"][name], np.full(x0.shape, ident, F), "reset of " + name)
    assert (tile_run["out"]["hfx_mean"] == F(-1e20)).sum() == 12          # skipped and not water in the land-use map: the fill


@pytest.mark.gpu
def test_probes_through_a_ring_follow_the_resort(oracle_run, tile_run, sorted_run):
    """37 points x 5 fields x 24 steps through a ring of 8 slots read back three times: the same cells of the oracle's per-step arrays."""
    pts = _probe_points()
    want = np.stack([np.stack([oracle_run["steps"][it][f].ravel()[pts] for f in PROBE_FIELDS]) for it in range(NSTEP)])
    assert want.shape == (24, 5, 37)
    assert_bits(tile_run["series"], want, "probes, tile order")
    assert_bits(sorted_run["series"], want, "probes, sorted layout")


def _block(ni, nj, xland, xice, thres=0.5):
    a = abi.StepArgs()
    a.ims = a.its = a.ids = 1
    a.jms = a.jts = a.jds = 1
    a.ime = a.ite = a.ide = ni
    a.jme = a.jte = a.jde = nj
    a.xland, a.xice, a.xice_thres = xland.data_ptr(), xice.data_ptr(), thres
    return a


def _shape_case(engine, ni, nj, nent, misalign=False, nlev_of=lambda f: 1, probes=False, seed=0):
    import torch
    r = np.random.default_rng(1000 + seed)
    ncol = ni * nj
    xland_h = r.choice(np.array([1.0, 2.0], dtype=F), ncol, p=[0.8, 0.2]).reshape(nj, ni)
    xice_h = r.choice(np.array([0.0, 1.0], dtype=F), ncol, p=[0.9, 0.1]).reshape(nj, ni)
    part = np_takes_part(xland_h, xice_h, 0.5)
    xland, xice = torch.from_numpy(xland_h).cuda(), torch.from_numpy(xice_h).cuda()
    ents, host = [], []
    for f in range(nent):
        nl = nlev_of(f)
        shape = (nj, ni) if nl == 1 else (nj, nl, ni)
        x, a0 = nasty(r, int(np.prod(shape))).reshape(shape), nasty(r, int(np.prod(shape))).reshape(shape)
        op = OPS[f % 5]
        xs = torch.from_numpy(x).cuda()
        if misalign:                                       # 4-byte but not 16-byte aligned: a slice of a larger buffer
            buf = torch.zeros(a0.size + 8, dtype=torch.float32, device="cuda")
            acc = buf[1:1 + a0.size].view(shape)
            acc.copy_(torch.from_numpy(a0))
            assert acc.data_ptr() % 16 == 4
        else:
            acc = torch.from_numpy(a0).cuda()
        ents.append((xs, acc, op, 3600.0))
        host.append((x, a0, op, nl))
    count = torch.zeros((nj, ni), dtype=torch.int32, device="cuda")
    pr = None
    if probes:
        npt, fields = min(ncol, 37), [e[0] for e in ents[:3]] or [xland, xice]
        cols = torch.from_numpy(r.integers(0, ncol, npt).astype(np.int32)).cuda()
        ring = torch.full((2, len(fields), npt), 7.0, dtype=torch.float32, device="cuda")
        pr = engine.history_probes(cols, fields, ring, slot=3)
    torch.cuda.synchronize()
    nrep = 2
    for _ in range(nrep):
        engine.history_step(ents, _block(ni, nj, xland, xice), probes=pr, count=count)
    engine.stream_sync()
    for f, (x, a0, op, nl) in enumerate(host):
        p = np.broadcast_to(part[:, None, :] if nl > 1 else part, a0.shape)
        want = a0
        for _ in range(nrep):
            want = np_apply(op, want, x, 3600.0, p)
        assert_bits(ents[f][1].cpu().numpy(), want, "%dx%d entry %d (%s, %d levels)" % (ni, nj, f, op, nl))
    assert np.array_equal(count.cpu().numpy(), np.where(part, nrep, 0))
    if probes:
        ring_h, cols_h = ring.cpu().numpy(), cols.cpu().numpy()
        assert (ring_h[0] == 7.0).all()                    # slot 3 % 2 = 1 was written, slot 0 was not
        for k, t in enumerate(fields):
            assert_bits(ring_h[1, k], t.cpu().numpy().ravel()[cols_h], "probe field %d" % k)


@pytest.mark.gpu
@pytest.mark.parametrize("ncol", [1, 63, 259])
def test_one_row_tiles_that_break_vectorisation(engine, ncol):
    _shape_case(engine, ncol, 1, 5, seed=ncol)
    _shape_case(engine, ncol, 1, 5, misalign=True, seed=ncol + 1)


@pytest.mark.gpu
def test_entry_counts_layers_and_probe_only_calls(engine):
    _shape_case(engine, 64, 3, 32, seed=1)                                             # n = 32
    _shape_case(engine, 64, 3, 32, misalign=True, seed=2)
    _shape_case(engine, 68, 5, 7, nlev_of=lambda f: (1, 4, 7)[f % 3], seed=3)         # layered, rows a multiple of four: vector path
    _shape_case(engine, 67, 5, 7, nlev_of=lambda f: (1, 4, 7)[f % 3], seed=4)          # layered, rows that are not: one column per thread
    _shape_case(engine, 259, 2, 0, probes=True, seed=5)                                # n = 0 with probes only
    _shape_case(engine, 259, 2, 4, probes=True, seed=6)                                # entries and probes in one launch
    _shape_case(engine, 256, 2, 4, probes=False, seed=7)                               # probes NULL


@pytest.mark.gpu
def test_invalid_calls_launch_nothing(engine):
    import torch
    lib = engine.lib
    ni, nj = 64, 2
    xland = torch.ones((nj, ni), device="cuda")
    xice = torch.zeros((nj, ni), device="cuda")
    x = torch.full((nj, ni), 2.0, device="cuda")
    acc = torch.full((nj, ni), 5.0, device="cuda")
    count = torch.zeros((nj, ni), dtype=torch.int32, device="cuda")
    ring = torch.full((2, 1, 4), 9.0, device="cuda")
    cols = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a = _block(ni, nj, xland, xice)

    def call(ents, n=None, probes=None, block=a):
        e = engine.history_entries(ents)
        rc = lib.noahmp_hip_history_step(e._n if n is None else n, e, C.byref(probes) if probes is not None else None, C.byref(block),
                                         count.data_ptr(), None)
        return rc, lib.noahmp_hip_last_error().decode()

    good = (x, acc, "sum", 0.0)
    rc, msg = call([good, (x, acc, 7, 0.0)])
    assert rc < 0 and "op" in msg
    rc, msg = call([good, (x, acc, -1, 0.0)])
    assert rc < 0 and "op" in msg
    rc, msg = call([good] * 33)
    assert rc < 0 and "entries" in msg
    rc, msg = call([good, (None, acc, "sum", 0.0)])
    assert rc < 0 and "NULL" in msg
    rc, msg = call([good, (x, None, "sum", 0.0)])
    assert rc < 0 and "NULL" in msg
    p = engine.history_probes(cols, [x], ring)
    p.npoint = 4097
    rc, msg = call([good], probes=p)
    assert rc < 0 and "probe points" in msg
    p = engine.history_probes(cols, [x], ring)
    p.nfield = 33
    rc, msg = call([good], probes=p)
    assert rc < 0 and "probe fields" in msg
    halo = _block(ni, nj, xland, xice)
    halo.its = 2
    rc, msg = call([good], block=halo)
    assert rc < 0 and "tile" in msg
    fl = (C.c_uint32 * 1)(abi.HIST_FIN["mean"])
    dst = (C.c_void_p * 1)(x.data_ptr())
    rc = lib.noahmp_hip_history_finish(1, engine.history_entries([good]), dst, fl, None, None, None, 16, -1e20, ni, nj, None)
    assert rc < 0 and "count" in lib.noahmp_hip_last_error().decode()
    engine.stream_sync()
    assert (acc == 5.0).all() and (count == 0).all() and (ring == 9.0).all() and (x == 2.0).all()
    rc, msg = call([good])                                 # ... and the same objects in a valid call
    engine.stream_sync()
    assert rc == 0 and (acc == 7.0).all() and (count == 1).all()


@pytest.mark.gpu
def test_history_between_asynchronous_steps(engine, tables, oracle_run):
    """Enqueue only: history_step between noahmp_hip_step_async calls, one noahmp_hip_sync at the end, gives the oracle's accumulators."""
    import torch
    s, _ = _start(tables)
    d = s.to_device("cuda:0")
    forc = []
    for it in range(1, NSTEP + 1):
        f = _forcing(s, it)
        forc.append({k: torch.from_numpy(f[k]).cuda() for k in FKEYS})
    acc = {"sfcrunoff": d.a["sfcrunoff"].clone(), "udrunoff": d.a["udrunoff"].clone()}
    count = torch.zeros((NJ, NI), dtype=torch.int32, device="cuda")
    ents = engine.history_entries([(d.a["runsfxy"], acc["sfcrunoff"], "sum_dt", DT), (d.a["runsbxy"], acc["udrunoff"], "sum_dt", DT)])
    torch.cuda.synchronize()
    args = d.step_args(1, 2000, 180.0)
    for it in range(1, NSTEP + 1):
        for k, v in forc[it - 1].items():
            setattr(args, k, v.data_ptr())
        args.itimestep = it
        engine.noahmplsm_async(args)
        engine.history_step(ents, args, count=count)
    st, step = engine.sync()
    assert st.code == 0 and step == -1
    part = oracle_run["part"]
    for name in acc:
        assert_bits(acc[name].cpu().numpy(), oracle_run["final"][name], name)
        assert_bits(d.a[name].cpu().numpy(), oracle_run["final"][name], name + " (the engine's own)")
    assert np.array_equal(count.cpu().numpy(), np.where(part, NSTEP, 0))


@pytest.mark.gpu
@_needs_flang()
def test_fortran_history_driver_equals_the_python_path(engine, tables):
    """tests/fortran/history_driver.f90 -- the device-resident loop with ACCPRCP / ACCECAN / ACCETRAN / ACCEDIR through the generated
    interfaces -- gives the four planes of the same chain driven from Python (History.add_reference_accumulators)."""
    import torch
    from tests.fortran import build_history
    from noahmp_amd.history import History
    lib = C.CDLL(build_history.build())
    lib.history_driver_run.argtypes = [C.POINTER(abi.StepArgs), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    engine.lib.noahmp_hip_set_tables(C.byref(tables[0]))
    r = np.random.default_rng(9)
    s = synth.mixed_small(tables[1], ni=96, nj=6, seed=19)
    synth.diurnal_forcing(s, 12, t_offset=s.t_offset)
    s["xlatin"] = r.uniform(-60.0, 70.0, size=(s.nj, s.ni)).astype(F)
    s["xland"][0, :5] = 2.0
    lon = r.uniform(-180.0, 180.0, size=(s.nj, s.ni)).astype(F)
    rain = np.where(r.random((s.nj, s.ni)) < 0.3, 4e-4, 0.0).astype(F)
    nsteps, iday0 = 30, 200
    # Python
    d = s.to_device("cuda:0")
    dlon, drain = torch.from_numpy(lon).cuda(), torch.from_numpy(rain).cuda()
    h = History(engine, d)
    h.add_reference_accumulators()
    torch.cuda.synchronize()
    args = d.step_args(1, 2000, 0.0)
    for n in range(nsteps):
        jul = engine.forcing_prep(d, dlon, drain, iday0 + n // 24, n % 24, first_step=(n == 0), wait=False)
        args.itimestep, args.julian = n + 1, jul
        engine.noahmplsm_async(args)
        h.step()
    st, _ = engine.sync()
    assert st.code == 0
    py = {it[0]: it[4].cpu().numpy() for it in h.items}
    # Fortran
    f = s.copy()
    acc4 = np.zeros((4, s.nj, s.ni), F)
    a = f.step_args(1, 2000, 0.0)
    rc = lib.history_driver_run(C.byref(a), lon.ctypes.data, rain.ctypes.data, nsteps, iday0, s.cfg.zlvl, acc4.ctypes.data)
    assert rc == 0, engine.lib.noahmp_hip_last_error().decode()
    for k, name in enumerate(("accprcp", "accecan", "accetran", "accedir")):
        assert_bits(acc4[k], py[name], name)
        assert np.count_nonzero(acc4[k]) > 50, name
    assert not acc4[:, 0, :5].any()                        # open water: never accumulated
    assert_bits(f["tslb"], d.a["tslb"].cpu().numpy(), "state")
