"""TEST INFRASTRUCTURE: compile + link tests/fortran/regions_driver.f90 with flang (modelled on build_history.py).

  libnoahmp_regions.so = noahmp_amd/fortran/module_sf_noahmpdrv_hip.F90 (modules noahmp_hip_abi / noahmp_hip_device: the generated
                         interfaces, among them noahmp_hip_region_plan / noahmp_hip_region_step)
                       + tests/fortran/regions_driver.f90 (dev_driver.f90's time loop with a basin series of RUNSFXY)
linked against libnoahmp_hip.so and oracle/_ref/libnoahmp_ref.so (the reference's table modules the shim `use`s)."""
import os
import subprocess

from . import build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = build_shim.ROOT
FC, REF = build_shim.FC, build_shim.REF
OUT = os.path.join(HERE, "_build", "regions")          # module files of its own: build_shim's are not touched
LIB = os.path.join(OUT, "libnoahmp_regions.so")


def available():
    return build_shim.available()


def build():
    os.makedirs(OUT, exist_ok=True)
    csrc = os.path.join(ROOT, "noahmp_amd", "csrc")
    srcs = [os.path.join(ROOT, "noahmp_amd", "fortran", "module_sf_noahmpdrv_hip.F90"), os.path.join(HERE, "regions_driver.f90")]
    if os.path.exists(LIB) and all(os.path.getmtime(s) <= os.path.getmtime(LIB) for s in srcs):
        return LIB
    cmd = [FC, "-cpp", "-fPIC", "-shared", "-O1", "-I" + os.path.join(REF, "mod_O0"), "-module-dir", OUT] + srcs + \
          ["-o", LIB, "-L" + REF, "-lnoahmp_ref", "-L" + csrc, "-lnoahmp_hip",
           "-Wl,-rpath," + REF, "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib/llvm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return LIB
