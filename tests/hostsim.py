"""Builds the host-logic test harness of tests/c: the product's per-stream host code (divans_amd/csrc/host_stream.cpp, ffi.cpp)
linked against tests/c/hostsim_device_stub.cpp, which answers the nine GPU entry points that code uses with the CPU oracle.
TEST INFRASTRUCTURE: nothing in divans_amd/ knows of it; it exists so that the call-by-call container logic and the parser of
untrusted input run in the "not gpu" tier, and under AddressSanitizer / UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "c", "_build")
# HOSTSIM_CXX / HOSTSIM_CC select the compilers (default g++ / gcc; /opt/rocm/lib/llvm/bin/clang++ is the host compiler hipcc uses for the product)
CXX = os.environ.get("HOSTSIM_CXX", "g++")
CC = os.environ.get("HOSTSIM_CC", "gcc")

CXX_SOURCES = ["divans_amd/csrc/host_stream.cpp", "divans_amd/csrc/ffi.cpp", "divans_amd/csrc/ir.cpp", "tests/c/hostsim_device_stub.cpp"]
C_SOURCES = ["oracle/cdf.c", "oracle/ans.c", "oracle/literal.c", "oracle/crc32c.c", "oracle/stream.c"]


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    deps = list(sources) + [os.path.join(ROOT, "divans_amd", "csrc", "host_stream.h"), os.path.join(ROOT, "oracle", "divans_oracle.h"),
                            os.path.join(ROOT, "include", "divans_gpu.h"), os.path.join(ROOT, "include", "divans_ffi.h"), os.path.join(ROOT, "include", "divans_ir.h"), os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def _objects(tag, flags):
    os.makedirs(OUT, exist_ok=True)
    objs = []
    for src in CXX_SOURCES + C_SOURCES:
        path = os.path.join(ROOT, src)
        obj = os.path.join(OUT, tag + "_" + os.path.basename(src) + ".o")
        if _newer(obj, [path]):
            cc = [CXX, "-std=c++17"] if src.endswith(".cpp") else [CC, "-std=c11"]
            subprocess.run(cc + flags + ["-fPIC", "-c", path, "-o", obj, "-I" + os.path.join(ROOT, "include")], check=True)
        objs.append(obj)
    return objs


def build_library():
    """tests/c/_build/libdivans_hostsim.so: the per-stream C ABI over the oracle-backed device stub, for ctypes."""
    lib = os.path.join(OUT, "libdivans_hostsim.so")
    objs = _objects("so", ["-O2", "-g", "-msse4.2"])
    if _newer(lib, objs):
        subprocess.run([CXX, "-shared", "-Wl,-Bsymbolic", "-o", lib] + objs + ["-lpthread"], check=True)   # its own divans_* symbols, whatever else the process has loaded
    return lib


def build_fuzzer():
    """tests/c/_build/hostsim_fuzz: tests/c/hostsim_fuzz.cpp with the same objects, everything under -fsanitize=address,undefined."""
    exe = os.path.join(OUT, "hostsim_fuzz")
    san = ["-O1", "-g", "-msse4.2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    objs = _objects("san", san)
    driver = os.path.join(ROOT, "tests", "c", "hostsim_fuzz.cpp")
    if _newer(exe, objs + [driver]):
        subprocess.run([CXX, "-std=c++17"] + san + ["-o", exe, driver] + objs + ["-I" + os.path.join(ROOT, "include"), "-lpthread"], check=True)
    return exe


def build_program(name, source, lang="c++", sanitize_main=True):
    """tests/c/_build/<name>: `source` (a caller of the per-stream C ABI) linked with the sanitized harness objects;
    sanitize_main=False leaves the caller itself uninstrumented (the reference's c/example.c trips UBSan in its own vec_u8.h).
    A `source` ending in .o is an object compiled elsewhere (oracle/Makefile's _ref/example_host.o) and is linked as it is."""
    exe = os.path.join(OUT, name)
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    objs = _objects("san", san + ["-msse4.2"])
    if _newer(exe, objs + [source]):
        obj = source
        if not source.endswith(".o"):
            obj = os.path.join(OUT, name + ".main.o")
            cc = [CXX, "-std=c++14"] if lang == "c++" else [CC, "-Wno-unused-result"]
            subprocess.run(cc + (san if sanitize_main else ["-O1", "-g"]) + ["-c", source, "-o", obj, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(source)], check=True)
        subprocess.run([CXX] + san + ["-o", exe, obj] + objs + ["-lpthread"], check=True)
    return exe


def build_thread_test():
    """tests/c/_build/hostsim_threads: tests/c/hostsim_threads.cpp and the harness objects under -fsanitize=thread."""
    exe = os.path.join(OUT, "hostsim_threads")
    san = ["-O1", "-g", "-msse4.2", "-fsanitize=thread", "-fno-omit-frame-pointer"]
    objs = _objects("tsan", san)
    driver = os.path.join(ROOT, "tests", "c", "hostsim_threads.cpp")
    if _newer(exe, objs + [driver]):
        subprocess.run([CXX, "-std=c++17"] + san + ["-o", exe, driver] + objs + ["-I" + os.path.join(ROOT, "include"), "-lpthread"], check=True)
    return exe


BATCH_SOURCE = "divans_amd/csrc/batch.cpp"


def build_batch_test(sanitizer="address,undefined"):
    """tests/c/_build/hostsim_batch_<tag>: tests/c/hostsim_batch.cpp + divans_amd/csrc/batch.cpp (compiled by g++ against
    tests/c/fakehip's stand-in for <hip/hip_runtime.h>) + the harness objects, under the given sanitizer."""
    tag = "tsan" if sanitizer == "thread" else "san"
    exe = os.path.join(OUT, "hostsim_batch_" + tag)
    san = ["-O1", "-g", "-msse4.2", "-fsanitize=" + sanitizer, "-fno-omit-frame-pointer"] + (["-fno-sanitize-recover=undefined"] if tag == "san" else [])
    objs = _objects(tag, san)
    batch_src = os.path.join(ROOT, BATCH_SOURCE)
    fake = os.path.join(ROOT, "tests", "c", "fakehip")
    batch_obj = os.path.join(OUT, tag + "_batch.cpp.o")
    if _newer(batch_obj, [batch_src, os.path.join(fake, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "divans_batch.h")]):
        subprocess.run([CXX, "-std=c++17"] + san + ["-fPIC", "-c", batch_src, "-o", batch_obj, "-I" + fake, "-I" + os.path.join(ROOT, "include")], check=True)
    driver = os.path.join(ROOT, "tests", "c", "hostsim_batch.cpp")
    if _newer(exe, objs + [batch_obj, driver]):
        subprocess.run([CXX, "-std=c++17"] + san + ["-o", exe, driver, batch_obj] + objs + ["-I" + os.path.join(ROOT, "include"), "-lpthread"], check=True)
    return exe


# ---- the launch contract of the batch C ABI (tests/c/README.md) ------------------------------------------------------------------
CAPI_SOURCES = ["capi.cpp", "lit_kernels.hip", "lit_decode2.hip", "lit_bucket.hip", "lit_bucket_mix.hip", "lit_bucket_ctx.hip", "lit_commands.hip"]


def find_hipcc():
    """the HIP compiler driver and its clang++, or (None, None): the launch-contract test skips without them"""
    import shutil
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            root = os.path.dirname(os.path.dirname(os.path.realpath(cand)))
            for clang in (os.path.join(root, "lib", "llvm", "bin", "clang++"), os.path.join(root, "llvm", "bin", "clang++")):
                if os.path.exists(clang):
                    return cand, clang
    return None, None


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _host_only_objects(hipcc, csrc, tag, sources, harness):
    """objects of `sources` (files of csrc) and `harness` (files of tests/c) compiled by hipcc for the HOST only, sanitized"""
    from concurrent.futures import ThreadPoolExecutor
    flags = ["--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g"] + [f for s in SAN for f in ("-Xarch_host", s)]
    headers = [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")] + [os.path.join(ROOT, "include", "divans_gpu.h"),
               os.path.join(ROOT, "tests", "c", "fakehip_rt.h"), os.path.abspath(__file__)]
    jobs = [(os.path.join(csrc, s), os.path.join(OUT, f"{tag}_{s}.o")) for s in sources]
    jobs += [(os.path.join(ROOT, "tests", "c", s), os.path.join(OUT, f"{tag}_{s}.o")) for s in harness]

    def compile_one(job):
        src, obj = job
        if not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in [src] + headers):
            subprocess.run([hipcc] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "c"), "-c", src, "-o", obj], check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(jobs), 8)) as ex:
        return list(ex.map(compile_one, jobs))


def _fatbin_stub(objs, tag):
    """every host-only object refers to the device code it would carry as __hip_fatbin_<hash>: data nobody reads here"""
    names = subprocess.run(["nm", "-u"] + objs, check=True, capture_output=True, text=True).stdout.split()
    fatbins = sorted({n for n in names if n.startswith("__hip_fatbin_")})
    stub = os.path.join(OUT, tag + "_fatbins.c")
    text = "".join(f"char {n}[16];\n" for n in fatbins)
    if not os.path.exists(stub) or open(stub).read() != text:
        with open(stub, "w") as f:
            f.write(text)
    return stub


def build_capi_contract(csrc=None, tag="contract"):
    """tests/c/_build/capi_contract: divans_amd/csrc/capi.cpp and the six .hip files compiled for the HOST only (hipcc
    --offload-host-only: the launchers and kernel stubs, no device code), tests/c/fakehip_rt.cpp in place of libamdhip64 and the
    driver tests/c/capi_contract.cpp (scenarios on the null stream, and streams_* on a caller's non-blocking stream: tests/c/README.md,
    "The stream model"), everything under -fsanitize=address,undefined.  A stand-alone program: nothing is preloaded.
    `csrc` selects another copy of the product sources (a copy with a deliberate break, to see a contract check fire)."""
    hipcc, clang = find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    csrc = csrc or os.path.join(ROOT, "divans_amd", "csrc")
    os.makedirs(OUT, exist_ok=True)
    objs = _host_only_objects(hipcc, csrc, tag, CAPI_SOURCES, ("fakehip_rt.cpp", "capi_contract.cpp"))
    stub = _fatbin_stub(objs, tag)
    exe = os.path.join(OUT, "capi_contract" if tag == "contract" else "capi_contract_" + tag)
    if _newer(exe, objs + [stub]):
        subprocess.run([clang] + SAN + ["-g", "-o", exe, "-x", "c", stub, "-x", "none"] + objs + ["-lpthread"], check=True)
    return exe


# ---- the device code on the CPU (tests/c/README.md, "Device code on the CPU") -------------------------------------------------------
SIMT_SOURCES = ["lit_decode2.hip"]        # the files whose KERNELS run on the lane-lockstep stand-in of tests/c/simt; the rest stay host-only


def build_device_code(csrc=None, tag="contract"):
    """tests/c/_build/device_code: as build_capi_contract, but SIMT_SOURCES are compiled as plain C++ by hipcc's clang++ against
    tests/c/simt/hip/hip_runtime.h (-DDIVANS_HOST_SIMT), so that their launches run the kernels' own source lane by lane on the
    runtime's memory; the driver is tests/c/device_code.cpp.  Everything under -fsanitize=address,undefined, nothing preloaded.  With
    the default sources the host-only objects are the ones build_capi_contract makes (same tag).  `csrc`: a copy with a deliberate
    break, to see a check fire."""
    hipcc, clang = find_hipcc()
    if not hipcc:
        raise RuntimeError("hipcc not found")
    csrc = csrc or os.path.join(ROOT, "divans_amd", "csrc")
    os.makedirs(OUT, exist_ok=True)
    objs = _host_only_objects(hipcc, csrc, tag, [s for s in CAPI_SOURCES if s not in SIMT_SOURCES], ("fakehip_rt.cpp",))
    stub = _fatbin_stub(objs, tag + "_simt")
    simt = os.path.join(ROOT, "tests", "c", "simt")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-DDIVANS_HOST_SIMT", "-D__HIP_PLATFORM_AMD__", "-Wno-unknown-attributes"] + SAN
    includes = ["-I" + os.path.join(simt), "-I" + rocm_include, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "c")]
    headers = [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")] + [os.path.join(simt, "hip", "hip_runtime.h"), os.path.join(simt, "simt_driver.h"),
               os.path.join(ROOT, "include", "divans_gpu.h"), os.path.join(ROOT, "tests", "c", "fakehip_rt.h"), os.path.abspath(__file__)]
    jobs = [(os.path.join(csrc, s), os.path.join(OUT, f"{tag}_simt_{s}.o")) for s in SIMT_SOURCES]
    jobs += [(os.path.join(simt, "simt.cpp"), os.path.join(OUT, "simt_simt.cpp.o")), (os.path.join(ROOT, "tests", "c", "device_code.cpp"), os.path.join(OUT, "simt_device_code.cpp.o"))]
    for src, obj in jobs:
        if not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in [src] + headers):
            subprocess.run([clang] + flags + includes + ["-c", src, "-o", obj], check=True)
        objs.append(obj)
    exe = os.path.join(OUT, "device_code" if tag == "contract" else "device_code_" + tag)
    if _newer(exe, objs + [stub]):
        subprocess.run([clang] + SAN + ["-g", "-rdynamic", "-o", exe, "-x", "c", stub, "-x", "none"] + objs + ["-lpthread", "-ldl"], check=True)
    return exe


# ---- the launch trace the program writes ------------------------------------------------------------------------------------------
LAUNCH_TRACE_GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace_small.json")


def trace_notes(trace, entry=None):
    return [r for r in trace if r.get("note") and (entry is None or r.get("entry") == entry)]


def small_trace_summary(trace):
    """what tests/golden/launch_trace_small.json holds: per codec and batch shape, the decode kernel, grid and LDS of decode_batch and
    decode_segments_batch, what divans_gpu_codec_info reports of the grid, and the pass every encode call ran"""
    out = {}
    for r in trace_notes(trace):
        case = r["case"]
        if r["entry"] in ("decode_batch", "decode_segments_batch"):
            out.setdefault(case, {})[r["entry"]] = {"kernel": r["kernel"], "grid": r["grid"]}
        elif r["entry"] == "info":
            out.setdefault(case, {})["info"] = {k: r[k] for k in ("n_streams", "resident_groups", "blocks", "rows_per_stream")}
        elif r["entry"] in ("encode_batch", "encode_segments_batch"):
            out.setdefault(case, {})[r["entry"]] = r["ran"]
    return out
