"""The decode kernels' OWN SOURCE on the CPU, every address checked (tests/c/README.md, "Device code on the CPU").

divans_amd/csrc/lit_decode2.hip is compiled for the host against the lane-lockstep stand-in of tests/c/simt; capi.cpp and the other
launchers are the host-only objects of the launch-contract tier, the memory is tests/c/fakehip_rt.cpp's.  tests/c/device_code.cpp
calls divans_gpu_lit_decode_batch / _decode_segments_batch as the GPU tests do, on the C oracle's bytes: what capi.cpp chooses --
instance, grid, LDS, cache organisation, tables -- is what runs.  The program is stand-alone, built with
-fsanitize=address,undefined; nothing is preloaded and nothing is loaded into Python.

Checked per launch: every decoded byte and every sentinel byte (equality), the status word, and that the instance the library names
is the one the stand-in ran.  Checked by construction: an LDS address outside the workgroup's allocation, a buffer access past
num_records ("SIMT FINDING"), a pointer that leaves its exact-size allocation (AddressSanitizer), undefined arithmetic (UBSan), a wave
whose lanes cannot go on.  Every case runs twice, fresh device memory and fresh LDS filled with 0xA7 and with 0x00: a result that
differs read memory nobody wrote.

Cases (tests/device_code_cases.py): per family of segment_cases.FAMILIES the short streams of plain_decoder_cases (output-group and
word-ring edges, the empty stream) without a list and segment_cases.shapes(small=True) with one; the stride families m5, m6, m7, m12 of
stride_bucketed_cases both ways; a segment that names block type 9; the 32 768 / 32 769-byte chunk seam once without mixing and once
with.  Cache sets: CM = 0, the high rows direct mapped (1 / 3) and 2-way (17 / 19), all four 2-way (21 / 27), the pinned organisation
(33), and the library's own choice.  `pytest -s` prints the instances that ran."""
import os
import re
import subprocess

import pytest

import device_code_cases as dc
import hostsim
import segment_cases as sc
import stride_bucketed_cases as sb

pytestmark = pytest.mark.skipif(hostsim.find_hipcc()[0] is None, reason="hipcc is not installed: the product's host code cannot be compiled")
_RAN = re.compile(r"^RAN (.+?) \| (.+?) \| (divans_hip::\S+<.*>) \| status (\d+) \| grid (\d+) \| out ([0-9a-f]{16})$")
POISON = ("0xA7", "0x00")


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _start(args):
    """one process per poison byte, side by side"""
    return [subprocess.Popen(args + [poison], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=ENV) for poison in POISON]


def _finish(procs, done):
    """-> ([(case, setting, kernel, status, grid, output hash)] per poison byte, [instances the stand-in ran])"""
    passes, instances = [], []
    for proc, poison in zip(procs, POISON):
        out, err = proc.communicate()
        assert proc.returncode == 0, f"poison {poison}: exit {proc.returncode}\n{out[-3000:]}\n{err[-6000:]}"
        assert "runtime error" not in err and "AddressSanitizer" not in err and "SIMT FINDING" not in err, err[-6000:]
        lines = out.splitlines()
        assert lines[0] == f"POISON {poison.lower()}" and lines[-1] == done, (lines[0], lines[-1])
        passes.append([])
        for line in lines:
            if line.startswith("RAN "):
                m = _RAN.match(line)
                assert m, line
                passes[-1].append((m.group(1), m.group(2), m.group(3), int(m.group(4)), int(m.group(5)), m.group(6)))
            elif line.startswith("SIMT RAN ") and len(passes) == 1:
                instances.append(line[len("SIMT RAN "):].split("  (")[0])
    return passes, instances


@pytest.fixture(scope="module")
def programs(tmp_path_factory, corpus, random_then_unicode, shuffle384):
    """the cases and the work-array shape, four processes side by side (two poison bytes each)"""
    exe = hostsim.build_device_code()
    d = tmp_path_factory.mktemp("device_code")
    cases = dc.all_cases((corpus, random_then_unicode, shuffle384))
    dc.write_cases(d / "cases.bin", cases)
    listed = dc.write_work(d / "work.bin", corpus)
    work = _start([exe, "work", str(d / "work.bin")])
    main = _start([exe, str(d / "cases.bin")])
    passes, instances = _finish(main, f"DONE {len(cases)} cases")
    wpasses, winstances = _finish(work, "DONE 1 cases")
    return dict(cases=cases, passes=passes, instances=instances, work=wpasses, work_instances=winstances, work_listed=listed)


@pytest.fixture(scope="module")
def run(programs):
    return programs


def _family(case_name):
    kind, fam = case_name.split("/")[:2]
    return sb.FAMILIES[fam] if kind.startswith("stride") or kind == "ragged37" else next(f for f in sc.FAMILIES if f.name == fam)


def test_every_case_decodes_under_both_poison_bytes(run):
    """the program ended well: every launch gave the literals back (the oracle's bytes in, equality out), the case's status word, no
    finding and no sanitizer report, and the same under 0xA7 and 0x00"""
    want = [(c["name"], s["label"]) for c in run["cases"] for s in c["settings"]]
    assert len(run["passes"]) == 2
    for lines in run["passes"]:
        assert [(name, label) for name, label, _, _, _, _ in lines] == want
    # kernel, status word and the hash of the whole output buffer: a difference is a read of memory nobody wrote
    assert run["passes"][0] == run["passes"][1], [(a, b) for a, b in zip(*run["passes"]) if a != b][:3]
    for c in run["cases"]:
        assert all(st == c["expect_status"] for name, _, _, st, _, _ in run["passes"][0] if name == c["name"])


def test_the_kernel_the_library_names_is_the_case_s_instance(run):
    """per case and setting divans_gpu_codec_last_decode_kernel (the program has checked that the stand-in ran exactly that instance
    once during the call): the family's (MM, CTXC, MIX, SEG) and, where the setting fixes the caches, the CM value"""
    lines = iter(run["passes"][0])
    for c in run["cases"]:
        fam = _family(c["name"])
        for k, s in enumerate(c["settings"]):
            name, label, kernel, _, grid, _ = next(lines)
            if name.startswith("ragged37/"):
                assert grid == 3, (name, kernel, grid)
            front, exact = dc.expected_kernel(c, fam, k)
            assert "lit_decode2_kernel_" in kernel and front in kernel, (name, label, kernel)
            if exact is not None:
                assert kernel == exact, (name, label, kernel, exact)
            else:
                assert kernel.endswith(", 0>") == (not fam.cached), (name, label, kernel)


def test_instances_covered(run):
    """what the tier covers, printed (pytest -s): every (MM, CTXC, MIX) triple without a list under CM = 0, high rows direct mapped,
    high rows 2-way and all four 2-way, with a list under the first three; the pinned instance"""
    ran = {i for i in run["instances"] if "lit_decode2_kernel_" in i}
    for i in sorted(run["instances"]):
        print("ran on the CPU:", i)
    want = set()
    for fam in sc.FAMILIES:
        mm = fam.mm if fam.mm >= 0 else -1
        for seg in (False, True):
            keys = ("none",) + ((("high", "high2") + (() if seg else ("full2",))) if fam.cached else ())
            for key in keys:
                want.add(f"divans_hip::lit_decode2_kernel_{'w7' if mm >= 0 else 'any'}<{mm}, {'true' if fam.ctxc else 'false'}, {'true' if fam.mix else 'false'}, "
                         f"{'true' if seg else 'false'}, {dc.cm_value(fam.mix, seg, key)}>")
    want.add("divans_hip::lit_decode2_kernel_w7<4, true, false, false, 33>")
    assert len(want) == 12 * 7 + 1
    assert want <= ran, sorted(want - ran)


def test_work_array_shape_of_m6_thresholds(programs):
    """part of the sequence of the FIRST occurrence of the open m6 fault, its decode half, in the threshold form:
    32 840 streams on a codec for 65 536-byte streams, the streams around every threshold of far_offset_cases.THRESHOLDS with their real
    lengths and every other stream empty, the oracle's bytes right-aligned in slots of divans_gpu_lit_encode_bound(65 536) (the last
    coded offset lies past 4 GiB), decode_batch and then decode_segments_batch on one codec, the library's own launch: the two instances
    of the record on 1280 workgroups, the literals back, status 0, no finding, the same under both poison bytes.  (The full form is the
    same program on device_code_cases.write_work(..., full=True).)"""
    assert programs["work_listed"] == sum(1 for i in dc.WORK_THRESHOLD_STREAMS if i % 6)
    assert programs["work"][0] == programs["work"][1]
    got = [(label, kernel, status, grid) for _, label, kernel, status, grid, _ in programs["work"][0]]
    assert got == [("decode_batch", dc.WORK_KERNELS[0], 0, dc.WORK_GRID), ("decode_segments_batch", dc.WORK_KERNELS[1], 0, dc.WORK_GRID)], got
