"""The batch C ABI's host code on a CPU-side HIP runtime (tests/c/README.md, "The launch contract"): divans_amd/csrc/capi.cpp and the
launchers of the six .hip files, compiled for the host only, run against tests/c/fakehip_rt.cpp, which tracks memory, records every
launch with its argument structs, checks each against the layouts of divans_amd/csrc/lit_kernels.h and fails on command.  The
program (tests/c/capi_contract.cpp) is stand-alone and built under ASan + UBSan; it writes its launch trace as JSON lines, read here.

A contract violation aborts the program with "CONTRACT VIOLATION ... kernel <name>: field <field>", a failed expectation of the
driver exits with "EXPECTATION FAILED"; either fails the test with the message."""
import json
import os
import subprocess

import numpy as np
import pytest

import encode_dispatch_cases as ed
import far_offset_cases as fo
import hostsim
import pyoracle as po

pytestmark = pytest.mark.skipif(hostsim.find_hipcc()[0] is None, reason="hipcc is not installed: the product's host code cannot be compiled")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = hostsim.build_capi_contract()
    d = tmp_path_factory.mktemp("capi_contract")
    configs = d / "configs.bin"
    configs.write_bytes(ed.config_records(po))
    sizes = d / "sizes.bin"
    sizes.write_bytes(np.array([fo.WORK_LENGTHS[i % len(fo.WORK_LENGTHS)] for i in range(fo.WORK_STREAMS)], np.uint32).tobytes())

    def run(scenario):
        trace = d / (scenario + ".jsonl")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        res = subprocess.run([exe, scenario, str(configs), str(trace), str(sizes)], capture_output=True, text=True, env=env)
        assert res.returncode == 0, f"{scenario}: exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
        assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-6000:]
        return [json.loads(line) for line in open(trace)]

    return run


@pytest.fixture(scope="module")
def small(program):
    return program("small")


def test_every_entry_point_at_small_shapes(small):
    """scenario 1: the contract held at every launch (the program ended well); the pass of every encode call is the dispatch table's (tests/encode_dispatch_cases.py)"""
    launches = [r for r in small if "seq" in r]
    kernels = {r["kernel"].split("<")[0] for r in launches}
    for family in ("lit_model_encode_kernel", "lit_decode2_kernel_any", "lit_decode_kernel", "lit_decode2_cmd_kernel", "lit_decode2_cmd_hist_kernel", "rans_encode",
                   "bucket_sort_kernel", "bucket_sort_stride_kernel", "bucket_chain_kernel", "mix_sort_kernel", "mix_chain_kernel", "mix_weights_kernel", "ctx_sort_kernel",
                   "mix_bt_sort_kernel", "lit_commands_prepare_kernel", "lit_commands_prepare_history_kernel", "pack_copy_kernel", "scan_sizes_kernel", "row_replay_kernel"):
        assert any(family in k for k in kernels), (family, sorted(kernels))
    for key, row in ed.TABLE.items():
        for shape in ("ragged37", "full_grid"):
            for path in (0, 1, 2):
                case = f"{key}/{shape}/path{path}"
                notes = [r for r in hostsim.trace_notes(small) if r["case"] == case]
                accepted = next(r["accepted"] for r in notes if r["entry"] == "set_encode_path")
                assert accepted == (path < 2 or row.accepted), case
                # where path 2 is refused the codec keeps the path it had: 1 in this walk, or the 2 that was accepted before the block types
                no_list, listed = row.ran[path]
                ran = {r["entry"]: r["ran"] for r in notes if "ran" in r}
                assert ran["encode_batch"] == no_list and ran["model_batch"] == no_list and ran["encode_packed"] == no_list, (case, ran)
                assert ran["encode_segments_batch"] == listed, (case, ran)
                assert ran["encode_commands_batch"] == listed and ran["encode_commands_history_batch"] == listed, (case, ran)
            dec = {r["entry"]: r for r in hostsim.trace_notes(small) if r["case"] == f"{key}/{shape}/decode"}
            full = shape == "full_grid"
            if not row.wrap:
                # one stream more than blocks2 * 16: the codec's own organisation (2-way without mixing) on the whole grid
                assert dec["decode_batch"]["kernel"].startswith("divans_hip::lit_decode2_kernel_"), dec
                assert (dec["decode_batch"]["grid"] % 256 == 0) == full, dec["decode_batch"]
                assert ", true, " in dec["decode_segments_batch"]["kernel"]
                assert "decode_commands_batch" in dec and "decode_commands_history_batch" in dec
            else:
                assert dec["decode_batch"]["kernel"].startswith("divans_hip::lit_decode_kernel<"), dec
                assert "decode_commands_batch" not in dec


def test_small_trace_is_the_committed_one(small):
    """tests/golden/launch_trace_small.json -- per codec and batch shape the pass of every encode call, the decode kernel and grid, the
    geometry divans_gpu_codec_info reports -- is what the harness gives today: a change of the dispatch has to change the file"""
    assert hostsim.small_trace_summary(small) == json.load(open(hostsim.LAUNCH_TRACE_GOLDEN))


def test_open_fault_sequence_replayed(program):
    """scenario 2: what test_work_arrays_past_4g does, with the family m6 behind the three it runs today -- 32 840 streams on codecs
    for 65 536-byte streams, 288 GiB of device memory -- under the contract.  The trace first reproduces what DESIGN.md section 4
    records of the real run (instance, LDS, grid, the fresh block under the second decode call); two things the record only supposed
    come out otherwise and are asserted as the replay has them: the tables are sized by the streaming encoder's grid of 1536
    workgroups (4.5 GiB, not 3.75), and m6's first tables are a fresh reservation -- every earlier codec is destroyed in mid-search on
    a block candidate and gives its mapped best back, so the pool is empty.  The contract then held at every launch of the sequence:
    the program ended well."""
    trace = program("m6")
    notes = [r for r in hostsim.trace_notes(trace) if r["case"].startswith("m6/work/path1")]
    dec = {r["entry"]: r for r in notes if r["entry"].startswith("decode")}
    assert dec["decode_segments_batch"]["kernel"] == "divans_hip::lit_decode2_kernel_any<-1, true, false, true, 17>"
    assert dec["decode_segments_batch"]["lds"] == 27648
    assert dec["decode_segments_batch"]["grid"] == 1280
    assert dec["decode_batch"]["kernel"] == "divans_hip::lit_decode2_kernel_any<-1, true, false, false, 17>" and dec["decode_batch"]["grid"] == 1280
    # the second decode call of one shape: placement_step moved the codec to a fresh hipMalloc block
    assert dec["decode_batch"]["tables"] == "chunks" and dec["decode_segments_batch"]["tables"] == "block"
    assert dec["decode_batch"]["tables_id"] != dec["decode_segments_batch"]["tables_id"]
    placement = next(r for r in notes if r["entry"] == "placement")
    assert placement["tried"] == 1 and placement["searching"] == 1
    ran = {r["entry"]: r["ran"] for r in notes if "ran" in r}
    assert ran == {"encode_batch": 1, "encode_segments_batch": 1, "model_batch": 1}
    # where the replay differs from what the record supposed
    assert placement["table_bytes"] == 1536 * 16 * 6144 * 32
    pools = hostsim.trace_notes(trace, "pool")
    assert [p["case"].split("/")[0] for p in pools] == ["simple", "mixing", "context_keyed", "m6"] and all(p["idle_ranges"] == 0 for p in pools)
    first_m6_launch = next(r for r in trace if "seq" in r and r["case"].startswith("m6/") and r["tables"] != "none")
    earlier = {r["tables_id"] for r in trace if "seq" in r and not r["case"].startswith("m6/") and r["tables"] != "none"}
    assert first_m6_launch["tables"] == "chunks" and first_m6_launch["tables_id"] not in earlier
    # every launch of the four codecs went through the contract: the streaming and the bucketed passes, both decoders
    assert {r["n_streams"] for r in trace if "seq" in r and r["n_streams"]} == {fo.WORK_STREAMS}


def test_placement_search(program):
    """scenario 3: scripted times; the fastest stays, two copies at most, no wait unless a call of another shape came between, block
    and chunk candidates alternate, the eager form, a candidate whose allocation fails"""
    trace = program("placement")
    calls = hostsim.trace_notes(trace, "search_call")
    assert [c["tables"] for c in calls] == ["chunks", "block", "chunks", "block", "block", "block"]
    assert max(c["copies"] for c in calls) == 2 and calls[-1]["copies"] == 1


def test_table_pool(program):
    """scenario 4"""
    program("pool")


def test_failure_sweep(program):
    """scenario 5: every injectable runtime call of decode_batch, encode_batch (paths 1 and 2) and the command calls fails in turn, on
    a small codec and on one with mapped tables under a placement search; and the case of its own: the launch, or the event record,
    behind placement_step's swap fails and the same shape is called again"""
    trace = program("failures")
    sweeps = hostsim.trace_notes(trace, "sweep")
    assert len(sweeps) == 10
    for s in sweeps:
        # `calls`: the injectable calls of the good run up to the end of its third call.  Every one of them is failed unless they are
        # thousands (then the first and last 50 and every 7th between); every injected failure fired; some were reported by a call,
        # the rest absorbed by a fallback the driver checks by name
        assert s["every_call_below"] >= 2000
        if s["calls"] < s["every_call_below"]:
            assert s["runs"] == s["calls"], s
        else:
            assert s["runs"] >= 100 + (s["calls"] - 100) // 7, s
        assert s["fired"] == s["runs"] and 0 < s["reported"] <= s["fired"], s
    assert {s["op"] for s in sweeps if s["mapped"]} == {s["op"] for s in sweeps if not s["mapped"]}
