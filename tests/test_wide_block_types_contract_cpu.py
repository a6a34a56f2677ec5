"""divans_gpu_codec_set_block_types above eight types on the CPU-side HIP runtime of the launch-contract test (tests/c/README.md): the
stand-alone program tests/c/wide_block_types_contract.cpp, built under ASan + UBSan by tests/wide_contract.py, makes every list call
on codecs in the wide context-table layout; tests/c/fakehip_rt.cpp checks each launch, the program the kernel names, the refusals and
the way back to eight types.  A contract violation aborts the program, a failed expectation exits with EXPECTATION FAILED: either
fails the test with the message."""
import json
import os
import subprocess

import pytest

import hostsim
import wide_contract

pytestmark = pytest.mark.skipif(hostsim.find_hipcc()[0] is None, reason="hipcc is not installed: the product's host code cannot be compiled")
LISTS = ("decode_segments_batch", "decode_commands_batch", "decode_commands_history_batch")


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    exe = wide_contract.build()
    path = tmp_path_factory.mktemp("wide_contract") / "trace.jsonl"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, f"exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-6000:]}"
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr[-6000:]
    assert "contract held" in res.stdout
    return [json.loads(line) for line in open(path)]


def _n_args(kernel):
    return kernel[kernel.index("<"):].count(",") + 1


def _wide(kernel):
    return _n_args(kernel) == (5 if "lit_decode2_cmd_" in kernel else 6)


def test_the_program_ran_clean_and_launched_the_wide_instances(trace):
    launches = [r for r in trace if "seq" in r]
    wide = {r["kernel"] for r in launches if ("lit_decode" in r["kernel"] or "lit_model_encode" in r["kernel"]) and _wide(r["kernel"])}
    assert all(k.endswith(", 1>") for k in wide), sorted(wide)
    for family in ("lit_model_encode_kernel", "lit_decode2_kernel_any", "lit_decode2_cmd_kernel", "lit_decode2_cmd_hist_kernel"):
        for mm in (4, -1):
            assert any(f"{family}<{mm}, false, " in k for k in wide), (family, mm, sorted(wide))
    assert not any("_w7<" in k for k in wide)


def test_wide_launches_stage_the_second_layout(trace):
    """2304 + 64 n bytes of context tables next to the row caches (and the mixing mask of a table-driven configuration): the LDS of
    the cache-less launches of the no-cache configuration is exactly that"""
    for n in (9, 256):
        sizes = {r["lds"] for r in trace if "seq" in r and r["case"].startswith(f"no_cache/bt{n}/") and "back_to_8" not in r["case"] and "lit_decode2" in r["kernel"] and _wide(r["kernel"])}
        assert sizes == {16 * 128 + 2304 + 64 * n + 8192}, (n, sizes)      # 16 word rings of 128 bytes, the tables, the mixing mask


def test_back_at_eight_types_the_old_instances_run(trace):
    notes = [r for r in trace if r.get("note") and r.get("entry") in LISTS]
    back = [r for r in notes if "/back_to_8/" in r["case"]]
    fresh = [r for r in notes if "/back_to_8/" not in r["case"] and not r["case"].startswith("constant")]
    assert len(back) == 8 * 3 and len(fresh) >= 8 * 3
    assert all(not _wide(r["kernel"]) for r in back), [r["kernel"] for r in back if _wide(r["kernel"])]
    assert all(_wide(r["kernel"]) for r in fresh), [r["kernel"] for r in fresh if not _wide(r["kernel"])]
    fused_lds = {r["lds"] for r in back if r["case"].startswith("no_cache/") and r["entry"] == "decode_segments_batch"}
    assert fused_lds == {16 * 128 + 256 + 2048 * 8 + 8192}, fused_lds
