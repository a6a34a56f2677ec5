"""The comparison helpers the GPU test families share (tests/gpu_harness.py), on hand-made numpy buffers: each one passes on equality
and fails -- naming the stream, or the sentinel -- on every kind of difference it exists to see.  A helper that stopped comparing would
let every GPU family pass; this file is what says so.  CPU tier: numpy only, no device, no library."""
import ast
import os

import numpy as np
import pytest

import gpu_harness as gh

SENTINEL = 0xEE
NAMES = ("alpha", "beta", "gamma")


def _layout():
    """three raw streams of 5, 8 and 3 bytes at offsets 4, 13 and 30 of a 40-byte buffer of sentinels"""
    offs, sizes = np.array([4, 13, 30], np.int64), np.array([5, 8, 3], np.int32)
    expect = np.full(40, SENTINEL, np.uint8)
    for k, (o, n) in enumerate(zip(offs, sizes)):
        expect[o:o + n] = np.arange(n, dtype=np.uint8) + 16 * (k + 1)
    streams = [dict(name=nm, cmds=np.zeros(k + 2, np.uint32), lit=np.zeros(4 + k, np.uint8)) for k, nm in enumerate(NAMES)]
    return dict(n=3, expect=expect, raw_off=offs, raw_sz=sizes), streams


def test_assert_raw_passes_on_equality_and_names_the_stream_and_byte():
    lay, streams = _layout()
    gh.assert_raw(lay["expect"].copy(), lay, streams, "equal")
    got = lay["expect"].copy(); got[13 + 3] ^= 1
    with pytest.raises(AssertionError, match=r"changed: stream 1 \(beta, 8 raw bytes\) wrong from its byte 3$"):
        gh.assert_raw(got, lay, streams, "changed")
    streams[1]["hist"] = np.zeros(7, np.uint8)      # history sizes are mentioned where the stream has a history, and only there
    with pytest.raises(AssertionError, match=r"stream 1 \(beta, 8 raw bytes, 7 history bytes\) wrong from its byte 3$"):
        gh.assert_raw(got, lay, streams, "changed")


def test_assert_raw_reports_an_overwritten_sentinel():
    lay, streams = _layout()
    for at in (0, 9, 12, 21, 39):       # in front, between the streams (the byte before stream 1, the byte behind it), behind
        got = lay["expect"].copy(); got[at] = 0x11
        with pytest.raises(AssertionError, match=rf"gap: sentinel byte {at} of the raw buffer overwritten with 17$"):
            gh.assert_raw(got, lay, streams, "gap")


def test_assert_raw_skips_a_stream_but_not_the_sentinels_next_to_it():
    lay, streams = _layout()
    got = lay["expect"].copy(); got[13:21] = 0
    gh.assert_raw(got, lay, streams, "skipped", skip=(1,))
    with pytest.raises(AssertionError, match=r"stream 1 \(beta"):
        gh.assert_raw(got, lay, streams, "not skipped")
    for at in (12, 21):
        bad = got.copy(); bad[at] = 0
        with pytest.raises(AssertionError, match=rf"sentinel byte {at} "):
            gh.assert_raw(bad, lay, streams, "skipped", skip=(1,))
    other = got.copy(); other[30] ^= 0x80        # ... nor another stream
    with pytest.raises(AssertionError, match=r"stream 2 \(gamma, 3 raw bytes\) wrong from its byte 0$"):
        gh.assert_raw(other, lay, streams, "skipped", skip=(1,))


def _coded():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, n, dtype=np.uint8) for n in (12, 20, 8)]


def test_assert_coded_sees_sizes_bytes_and_literal_sizes():
    _, streams = _layout()
    ref = _coded()
    res = lambda coded, lit_sz=(4, 5, 6): dict(coded=coded, lit_sz=np.array(lit_sz, np.int32))
    gh.assert_coded(res([c.copy() for c in ref]), streams, ref, "equal")
    longer = [c.copy() for c in ref]; longer[1] = np.concatenate([ref[1], ref[1][:4]])      # a size mismatch with an equal prefix
    shorter = [c.copy() for c in ref]; shorter[1] = ref[1][:16].copy()
    changed = [c.copy() for c in ref]; changed[1][19] ^= 1
    for what, got in (("longer", longer), ("shorter", shorter), ("changed", changed)):
        with pytest.raises(AssertionError, match=rf"{what}: stream 1 \(beta, 3 commands\) differs from the oracle$"):
            gh.assert_coded(res(got), streams, ref, what)
        gh.assert_coded(res(got), streams, ref, what, skip=(1,))
    with pytest.raises(AssertionError, match=r"stream 2 \(gamma, 4 commands\): literal size 7, the stream has 6$"):
        gh.assert_coded(res([c.copy() for c in ref], (4, 5, 7)), streams, ref, "literal size")
    streams[0]["hist"] = np.zeros(9, np.uint8)
    with pytest.raises(AssertionError, match=r"stream 0 \(alpha, 2 commands, 9 history bytes\): literal size 0, "):
        gh.assert_coded(res([c.copy() for c in ref], (0, 5, 6)), streams, ref, "literal size")


@pytest.mark.parametrize("named", [True, False])
def test_assert_same_sees_sizes_and_bytes(named):
    ref = _coded()
    streams = [(nm, np.zeros(10 * (k + 1), np.uint8), np.zeros(k + 1, np.uint64)) for k, nm in enumerate(NAMES)] if named else None
    who = r"beta, 20 bytes, 2 segments, " if named else ""
    gh.assert_same([c.copy() for c in ref], ref, streams, "equal")
    longer = [c.copy() for c in ref]; longer[1] = np.concatenate([ref[1], ref[1][:4]])
    shorter = [c.copy() for c in ref]; shorter[1] = ref[1][:16].copy()
    changed = [c.copy() for c in ref]; changed[1][0] ^= 0x80
    for what, got, n in (("longer", longer, 24), ("shorter", shorter, 16), ("changed", changed, 20)):
        with pytest.raises(AssertionError, match=rf"{what}: stream 1 \({who}{n} bytes against 20\) differs"):
            gh.assert_same(got, ref, streams, what)
        gh.assert_same(got, ref, streams, what, skip=(1,))
    with pytest.raises(AssertionError, match=r"fewer: 2 streams against 3 expected$"):
        gh.assert_same([c.copy() for c in ref[:2]], ref, streams, "fewer")
    if named:       # the reference may hold more streams than the batch (a batch of the first streams of a case), never fewer
        gh.assert_same([c.copy() for c in ref[:2]], ref, streams[:2], "the first two")
        with pytest.raises(AssertionError, match=r"3 streams against 2 expected$"):
            gh.assert_same([c.copy() for c in ref], ref[:2], streams, "short reference")


def test_split_outputs_returns_what_offsets_and_sizes_describe():
    out = np.arange(64, dtype=np.uint8)
    outs = dict(out=out, offsets=np.array([20, 0, 40], np.int64), sizes=np.array([12, 0, 8], np.int32), slot=20)
    got = gh.split_outputs(outs, 3)
    assert [g.tolist() for g in got] == [list(range(20, 32)), [], list(range(40, 48))]
    assert [g.tolist() for g in gh.split_outputs(outs, 1)] == [list(range(20, 32))]


def test_assert_decoded_sees_a_wrong_byte_and_bytes_behind_the_batch():
    streams = [(nm, np.arange(n, dtype=np.uint8) + 1, np.zeros(2, np.uint64)) for nm, n in zip(NAMES, (5, 8, 3))]
    tin = dict(off=np.array([0, 5, 13], np.int64), total=16)
    back = np.concatenate([s[1] for s in streams] + [np.zeros(8, np.uint8)])
    gh.assert_decoded(back, tin, streams, "equal")
    bad = back.copy(); bad[5 + 6] = 0
    with pytest.raises(AssertionError, match=r"stream 1 \(beta, 8 bytes, 2 segments\) decoded wrong from byte 6$"):
        gh.assert_decoded(bad, tin, streams, "changed")
    gh.assert_decoded(bad, tin, streams, "changed", skip=(1,))
    bad = back.copy(); bad[17] = 1
    with pytest.raises(AssertionError, match="bytes written behind the batch"):
        gh.assert_decoded(bad, tin, streams, "behind")


def test_assert_plain_decoded_sees_a_wrong_byte_and_a_written_sentinel():
    lay, _ = _layout()
    streams = [(nm, lay["expect"][o:o + n].copy()) for nm, o, n in zip(NAMES, lay["raw_off"], lay["raw_sz"])]
    case = dict(streams=streams, coded=_coded(), lit=(lay["expect"], None, lay["raw_off"], lay["raw_sz"]))
    gh.assert_plain_decoded(lay["expect"].copy(), case, "equal")
    bad = lay["expect"].copy(); bad[31] ^= 2
    with pytest.raises(AssertionError, match=r"stream 2 \(gamma, 3 bytes, 2 coded words\) decoded wrong from byte 1$"):
        gh.assert_plain_decoded(bad, case, "changed")
    bad = lay["expect"].copy(); bad[29] = 0
    with pytest.raises(AssertionError, match=r"sentinel byte 29 of 40 written to$"):
        gh.assert_plain_decoded(bad, case, "gap")


def test_the_harness_loads_no_device_code_when_imported():
    """torch, divans_amd and the oracle are imported inside functions only: the CPU tier imports the module, and so does collection"""
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_harness.py")).read())
    top = {a.name for node in tree.body if isinstance(node, ast.Import) for a in node.names} | {node.module for node in tree.body if isinstance(node, ast.ImportFrom)}
    assert top == {"numpy", "bucketed_segment_cases", "command_cases", "history_cases", "segment_cases"}, top
