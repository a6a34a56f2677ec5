"""The command lists of tests/command_cases.py without a GPU: the Python executor against the product's own IR walk on the six golden
IRs (CommandIR.device_commands() + the IR's literals must give expand() and exactly literal_segments()), the directed batch through
the C oracle and back, and the record's size."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import command_cases as cc
import irtext
import pyoracle as po
import segment_cases as sc

NAMES = ["alice29", "alice29-q11", "alice29-priors", "asyoulik", "random_then_unicode", "ends_with_truncated_dictionary"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


@pytest.mark.parametrize("name", NAMES)
def test_executor_on_device_commands_gives_the_ir_walk(name):
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text(name))
    cmds, ins = ir.device_commands()
    lit, segs = ir.literal_segments()
    assert cmds.dtype == cc.CMD_DTYPE == da.CMD_DTYPE
    assert cmds.size == ir.count("literal") + ir.count("copy") + ir.count("dict")
    assert int((cmds["kind"] == cc.LITERAL).sum()) == ir.count("literal") and int((cmds["kind"] == cc.COPY).sum()) == ir.count("copy")
    assert int((cmds["kind"] == cc.INSERT).sum()) == ir.count("dict") and not cmds["reserved"].any()
    assert ins.size == int(cmds["len"][cmds["kind"] == cc.INSERT].sum())
    raw, got = cc.execute(cmds, lit, ins)
    ref = ir.expand()
    assert raw.size == ref.size and (raw == ref).all()
    assert got.size == segs.size and (got["len"] == segs["len"]).all() and (got["btype"] == segs["btype"]).all() and (got["last8"] == segs["last8"]).all()
    ir.close()


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_directed_batch_round_trips_through_the_oracle(fam, sources):
    import divans_amd as da
    g, o = fam.pair(da, po)
    streams = cc.directed(fam, sources)
    assert len(streams) == 40 and len(set(s["name"] for s in streams)) == 40
    for s in streams:
        segs = s["segs"]
        assert int(segs["len"].sum()) == s["lit"].size and (segs["btype"] < fam.n_btypes).all()
        coded = po.lit_segments_encode(o, s["lit"], segs["len"], segs["btype"], segs["last8"])
        assert coded.size % 4 == 0
        back = po.lit_segments_decode(o, coded, s["lit"].size, segs["len"], segs["btype"], segs["last8"])
        assert (back == s["lit"]).all(), s["name"]
    lay = cc.layout(streams, [np.zeros(4 * (i % 3), np.uint8) for i in range(len(streams))])
    assert sorted(set(int(x) % 16 for x in lay["raw_off"])) == list(range(16))
    assert sorted(set(int(x) % 16 for x in lay["coded_off"])) == [0, 4, 8, 12]
    assert all(int(x) % 2 == 1 for x in lay["ins_off"])
    for i, s in enumerate(streams):       # sentinels in front of and behind every raw range
        ro = int(lay["raw_off"][i])
        assert lay["expect"][ro - 1] == cc.RAW_SENTINEL and lay["expect"][ro + s["raw"].size] == cc.RAW_SENTINEL


def test_faulty_lists_are_faulty_for_the_executor_too(sources):
    fam = sc.FAMILIES[0]
    v, _ = cc.victim_base(fam, sources)
    for what, cmds, nlit, bit in cc.faulty_lists(fam, v):
        lit = np.resize(v["lit"], nlit)
        try:
            raw, segs = cc.execute(cmds, lit, v["ins"], raw_size=v["raw"].size)
        except ValueError:
            continue
        assert raw.size != v["raw"].size or (segs["btype"] >= fam.n_btypes).any(), what


def test_command_record_is_16_bytes(tmp_path):
    import divans_amd as da
    assert ctypes.sizeof(da.LitCommand) == 16 and da.CMD_DTYPE.itemsize == 16 and cc.CMD_DTYPE.itemsize == 16
    assert (da.CMD_COPY, da.CMD_INSERT, da.CMD_LITERAL) == (cc.COPY, cc.INSERT, cc.LITERAL) and da.STATUS_BAD_COMMAND == cc.BAD_COMMAND
    src = tmp_path / "size.c"
    src.write_text('#include "divans_gpu.h"\n'
                   "typedef char size_is_16[sizeof(divans_lit_command) == 16 ? 1 : -1];\n"
                   "typedef char kinds[DIVANS_CMD_COPY == 0 && DIVANS_CMD_INSERT == 1 && DIVANS_CMD_LITERAL == 3 && DIVANS_GPU_STATUS_BAD_COMMAND == 16u ? 1 : -1];\n"
                   "int main(void) { return 0; }\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
