"""The batch C ABI on a CALLER'S NON-BLOCKING stream, on the CPU-side HIP runtime (tests/c/README.md, "The stream model").

tests/test_capi_launch_contract_cpu.py drives every codec on the null stream, which serialises against everything else and so
hides any ordering the library forgets.  Here the same program (tests/c/capi_contract.cpp, stand-alone, ASan + UBSan, nothing
preloaded) creates its codecs on a stream made with hipStreamNonBlocking.  On such a stream the runtime keeps every launch, copy,
fill, event record and wait as an entry of its stream's queue with the ledger ranges it reads and writes; what the host can see of
an entry (the destination of a device-to-host copy) arrives only when something completes the entry; and an operation that meets an
entry of ANOTHER stream -- or a synchronous copy, fill, free or map that meets any entry in flight -- on the same bytes, one of the
two writing, with no event, wait or synchronisation between them, ends the program with `CONTRACT VIOLATION ... field order`
(`field lifetime` for a free or an unmap).  The driver's effects write values that differ from call to call, and every value a call
reads back (totals, sizes, offsets, the status word, coded and decoded bytes) is compared with its own launch's."""
import json
import os
import subprocess

import pytest

import encode_dispatch_cases as ed
import hostsim
import pyoracle as po

pytestmark = pytest.mark.skipif(hostsim.find_hipcc()[0] is None, reason="hipcc is not installed: the product's host code cannot be compiled")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = hostsim.build_capi_contract()
    d = tmp_path_factory.mktemp("caller_streams")
    configs = d / "configs.bin"
    configs.write_bytes(ed.config_records(po))

    def run(scenario):
        trace = d / (scenario + ".jsonl")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        res = subprocess.run([exe, scenario, str(configs), str(trace)], capture_output=True, text=True, env=env)
        assert res.returncode == 0, f"{scenario}: exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
        assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-6000:]
        return [json.loads(line) for line in open(trace)]

    return run


def test_every_entry_point_on_a_non_blocking_stream(program):
    """scenario 1's call table -- every device-pointer entry point on the ten codecs of the dispatch table, at both shapes, the
    grown work buffers, the big caches -- with every codec on the caller's stream; then, on three configurations, the status calls
    (status, status_async into page-locked memory, clear_status between a failing and a later failing call, the per-stream
    flags), pack_streams, and every setter called behind launches nothing has waited for.  The dispatch does not depend on the
    stream: the trace's summary is the committed one of the null stream."""
    trace = program("streams_small")
    assert hostsim.small_trace_summary(trace) == json.load(open(hostsim.LAUNCH_TRACE_GOLDEN))
    cases = {r["case"] for r in trace if "seq" in r}
    for name in ("simple", "mixing", "context_keyed"):
        assert f"{name}/setters_in_flight" in cases
    assert "simple/status" in cases and "mixing/status" in cases


def test_placement_search_on_a_non_blocking_stream(program):
    """scenario 3 on the caller's stream: the table swaps of the call-by-call search, the eager form and a failed candidate free and
    map table memory between launches of a stream nothing else serialises; the search's own waits are the only ones it gets"""
    trace = program("streams_placement")
    calls = [r for r in trace if r.get("note") and r.get("entry") == "search_call"]
    assert [c["tables"] for c in calls] == ["chunks", "block", "chunks", "block", "block", "block"]
    assert max(c["copies"] for c in calls) == 2 and calls[-1]["copies"] == 1


def test_host_buffer_entry_points_on_a_non_blocking_stream(program):
    """encode_host, encode_host_chunks, decode_host, both pipelined calls with 1, 3 and 7 slices into page-locked and pageable
    buffers, stream_begin / _encode / _finish, stream_decode_begin / _decode and the selftest calls, two rounds on one codec: each
    returns the total, sizes, offsets, chunk sizes, bytes and error code of its own launches"""
    trace = program("streams_host")
    cases = {r["case"] for r in trace if "seq" in r}
    for name in ("simple", "mixing"):
        for entry in ("encode_host", "encode_host_chunks", "decode_host", "pipelined/1_slices_pinned", "pipelined/3_slices_pageable", "pipelined/7_slices_pinned",
                      "stream_encode", "stream_decode", "selftests"):
            assert f"{name}/host/{entry}" in cases, (name, entry, sorted(cases))
