"""The expectations of tests/test_gpu_command_encode.py without a GPU: prepare() of tests/command_encode_cases.py -- the restatement of
the device step that turns raw bytes and a command list into literals and segments -- gives back exactly what the executor of
tests/command_cases.py derived the raw bytes from, agrees with the product's own IR walk on the six golden IRs, and names the listed
status bit for every faulty input.  Guards the expectations; passes with or without the device entry point."""
import numpy as np
import pytest

import command_cases as cc
import command_encode_cases as ce
import irtext
import pyoracle as po
import segment_cases as sc

NAMES = ["alice29", "alice29-q11", "alice29-priors", "asyoulik", "random_then_unicode", "ends_with_truncated_dictionary"]


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _assert_inverts_the_executor(streams, n_btypes):
    for s in streams:
        got = ce.prepare(s["cmds"], s["raw"], s["ins"], n_btypes, max(s["lit"].size, 16))
        assert ce.same_lists(got, s["lit"], s["segs"]), s["name"]


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_prepare_inverts_the_executor_on_the_directed_batches(fam, sources):
    _assert_inverts_the_executor(cc.directed(fam, sources), fam.n_btypes)
    edges = ce.count_edges(fam, sources)
    assert len(set(s["name"] for s in edges)) == len(edges)
    _assert_inverts_the_executor(edges, fam.n_btypes)
    by = {s["name"]: s for s in edges}
    assert by["count0"]["raw"].size == 0 and by["count1000"]["segs"].size > 300
    s = by["last8_spans_three_commands"]        # the context of its second Literal command: 3 literal, 3 copied, 2 inserted bytes
    assert bytes(int(s["segs"]["last8"][1]).to_bytes(8, "little")) == bytes(s["raw"][17:25]) and s["cmds"]["len"].tolist() == [20, 3, 2, 9]
    s = by["second_literal_near_start"]
    assert int(s["segs"]["last8"][1]) >> 24 == int.from_bytes(bytes(s["raw"][:5]), "little") and int(s["segs"]["last8"][1]) & 0xffffff == 0


def test_prepare_inverts_the_executor_on_ragged_prefixes():
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text("alice29-priors"))
    cmds, ins = ir.device_commands()
    lit, _ = ir.literal_segments()
    _assert_inverts_the_executor(cc.prefix_streams(cmds, lit, ins, 40), ir.num_block_types)
    ir.close()


@pytest.mark.parametrize("name", NAMES)
def test_prepare_gives_the_ir_walk(name):
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text(name))
    cmds, ins = ir.device_commands()
    lit, segs = ir.literal_segments()
    got = ce.prepare(cmds, ir.expand(), ins, ir.num_block_types, lit.size)
    assert ce.same_lists(got, lit, segs)
    ir.close()


@pytest.mark.parametrize("fam", [sc.FAMILIES[0], sc.FAMILIES[-1]], ids=repr)
def test_faulty_inputs_raise_their_bit(fam, sources):
    import divans_amd as da
    g, o = fam.pair(da, po)
    victim, _ = cc.victim_base(fam, sources)
    inputs = ce.faulty_inputs(fam, victim, sources)
    assert len(inputs) == 20 and sum(e["bit"] == 0 for e in inputs) == 2
    for e in inputs:
        got = ce.prepare(e["cmds"], e["raw"], e["ins"], fam.n_btypes, e["lit_cap"])
        if e["bit"]:
            assert got == e["bit"], (e["what"], got)
            continue
        assert ce.same_lists(got, e["lit"], e["segs"]), e["what"]
        lit, segs = got
        coded = po.lit_segments_encode(o, lit, segs["len"], segs["btype"], segs["last8"])
        back = po.lit_segments_decode(o, coded, lit.size, segs["len"], segs["btype"], segs["last8"])
        assert (back == lit).all(), e["what"]
    changed = inputs[-1]
    assert changed["what"] == "byte inside the last literal command changed" and int((changed["lit"] != victim["lit"]).sum()) == 1
    # ... and a changed byte that a copy reads is caught whichever side of the copy it lies on
    assert isinstance(ce.prepare(victim["cmds"], victim["raw"], victim["ins"], fam.n_btypes, 64), tuple)
    raw = victim["raw"].copy(); raw[25] ^= 1        # read by copy (20, 10): raw[35] no longer equals it
    assert ce.prepare(victim["cmds"], raw, victim["ins"], fam.n_btypes, 64) == cc.BAD_COMMAND
