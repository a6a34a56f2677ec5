"""Builds tests/c/_build/wide_block_types_contract: the driver tests/c/wide_block_types_contract.cpp linked with the host-only objects
of the batch C ABI and the recording HIP runtime that hostsim.build_capi_contract() compiles (capi.cpp and the .hip files under
--offload-host-only, tests/c/fakehip_rt.cpp), in place of that builder's own driver.  Everything is compiled with
-fsanitize=address,undefined through -Xarch_host; the result is a stand-alone program: nothing is preloaded, nothing is loaded into Python."""
import os
import subprocess

import hostsim

DRIVER = os.path.join(hostsim.ROOT, "tests", "c", "wide_block_types_contract.cpp")


def build():
    hipcc, clang = hostsim.find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    hostsim.build_capi_contract()       # the objects (and its own program, which test_capi_launch_contract_cpu.py runs)
    out = hostsim.OUT
    objs = [os.path.join(out, f"contract_{s}.o") for s in hostsim.CAPI_SOURCES + ["fakehip_rt.cpp"]]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    flags = ["--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g"] + [f for s in san for f in ("-Xarch_host", s)]
    csrc = os.path.join(hostsim.ROOT, "divans_amd", "csrc")
    deps = [DRIVER, os.path.join(csrc, "lit_kernels.h"), os.path.join(hostsim.ROOT, "include", "divans_gpu.h"),
            os.path.join(hostsim.ROOT, "tests", "c", "fakehip_rt.h"), os.path.abspath(__file__)]
    obj = os.path.join(out, "wide_block_types_contract.cpp.o")
    if not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in deps):
        subprocess.run([hipcc] + flags + ["-I" + os.path.join(hostsim.ROOT, "include"), "-I" + os.path.join(hostsim.ROOT, "tests", "c"), "-c", DRIVER, "-o", obj], check=True)
    exe = os.path.join(out, "wide_block_types_contract")
    stub = os.path.join(out, "contract_fatbins.c")      # the __hip_fatbin_<hash> symbols of the host-only objects: data nobody reads here
    if hostsim._newer(exe, objs + [obj, stub]):
        subprocess.run([clang] + san + ["-g", "-o", exe, "-x", "c", stub, "-x", "none", obj] + objs + ["-lpthread"], check=True)
    return exe
