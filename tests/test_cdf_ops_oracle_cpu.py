"""The expected values of the device CDF-operation sweeps (tests/test_gpu_cdf_ops_sweeps.py), double-checked without a GPU:
the C script interpreter (oracle/cdf_ops.c: orc_cdf_ops_run, calls of the oracle's own functions only) against the independent
Python restatement (ref_restatement.py) on a thinned version of every sweep, and the generators' own promises."""
import numpy as np
import pytest

import cdf_ops_sweeps as sw


def test_speeds_are_supported_and_follow_one_trajectory():
    import divans_amd as da
    for sp in sw.all_speeds() + [(1, 16384), (8160, 1), (8100, 16384), (4096, 16384)]:
        assert da.speed_supported(*sp), sp
        tr = sw.trajectory(*sp)
        # the oracle's blend walks the same totals: 200 updates of symbol 15 from the default row
        rec = sw.oracle_run([(0, 15, *sp)] * 200)
        want = [t for t, _ in tr]
        while len(want) < 201:
            want.append((lambda n: (n + 16) - ((n + 16) >> 2) if n >= sp[1] else n)(want[-1] + sp[0]))
        assert [int(v) for v in rec[:, 15]] == want[1:201], sp


def test_row_shapes_cover_the_edges():
    rows = sw.read_rows()
    assert len(rows) >= 32
    totals = {r[15] for _, r in rows}
    assert set(sw.SPECIAL_TOTALS) <= totals
    for shape in sw.SHAPES:
        assert sum(n.startswith(shape) for n, _ in rows) >= 3, shape
    assert sw.make_row("low", 32767) == list(range(1, 16)) + [32767]
    assert sw.make_row("high", 32767) == list(range(32752, 32768))
    assert len(sw.row_pairs()) >= 64


@pytest.mark.parametrize("name", ["blend", "search", "search_encoder", "average", "mixed_encode", "state", "mixed_decode", "weights"])
def test_c_interpreter_agrees_with_the_python_restatement(name):
    ops, exp, bounds = sw.sweep(name)          # runs the restatement on the thinned sweep and asserts agreement
    assert ops.shape[0] == exp.shape[0] == bounds[-1] and ops.shape[0] > 1000
    if name.startswith("search"):
        for i in range(len(bounds) - 1):
            sw.check_search_records(ops[bounds[i]:bounds[i + 1]], exp[bounds[i]:bounds[i + 1]])


def test_existing_reference_unit_scripts_agree():
    # the four scripts tests/test_gpu_reference_unit_tests.py runs on the device, in full, on both CPU opinions
    for make in (sw.script_operation_test_helper, sw.script_declare_common_tests, sw.script_lcg_sample_run, sw.script_weights_update_sequences):
        sw.second_opinion(make())


def test_state_step_of_the_decoder_is_the_factored_function():
    # orc_ans_get_nibble and op 9 go through the same orc_ans_advance_state: a stream the oracle encodes still decodes
    import pyoracle as po
    data = np.arange(4096, dtype=np.uint32).astype(np.uint8)
    for cfg in (po.config_simple(), po.config_context_mixing()):
        assert (po.lit_decode(cfg, po.lit_encode(cfg, data), data.size) == data).all()
