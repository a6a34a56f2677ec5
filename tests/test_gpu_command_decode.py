"""divans_gpu_lit_decode_commands_batch: general streams decoded from their command lists, the decoder running the Copy / Insert
commands itself and taking every Literal command's context from its own output.  The coded bytes are the C ORACLE's (made from the
segments the Python executor of tests/command_cases.py derives; tests/test_command_cases_cpu.py guards both), the expectation is
the executor's raw bytes inside a buffer of sentinels, compared whole.

Two long streams carry the rANS chunk seam: one cannot hold both a command boundary exactly on literal 32 768 and a Literal command
that spans it."""
import numpy as np
import pytest

import command_cases as cc
import gpu_harness as gh
import irtext
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
NAMES = ["alice29", "alice29-q11", "alice29-priors", "asyoulik", "random_then_unicode", "ends_with_truncated_dictionary"]
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _case(fam, sources):
    """the family's configurations, its directed batch, the oracle's bytes and the batch's layout: computed once, shared, never written to"""
    if fam.name not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        streams = cc.directed(fam, sources)
        coded = gh.oracle_bytes(o, streams)
        _CASES[fam.name] = (g, o, streams, coded, cc.layout(streams, coded))
    return _CASES[fam.name]


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_directed_batch(fam, sources):
    """grids of two workgroups and of one (16 resident groups: every group runs two or three streams in a row, so cursor, raw position and
    word ring are reset), then the codec's own grid, and once under a cache organisation the commands call has to reduce"""
    import torch
    import divans_amd as da
    g, o, streams, coded, lay = _case(fam, sources)
    t = gh.to_device(torch, lay)
    codec = gh.codec_for(da, fam, g, lay["lit_longest"])
    steps = [("2 workgroups", lambda c: c.set_geometry(blocks=2)), ("1 workgroup", lambda c: c.set_geometry(blocks=1)),
             ("direct-mapped decoder asked for", lambda c: c.set_decoder(2))]
    if fam.cached:
        steps.append(("tiny 2-way caches with low-row caches asked for", lambda c: c.set_decoder(3, (8, 8, 8, 8), (5, 5, 5, 5), blocks=2)))
    for what, setup in steps:
        setup(codec)
        st, raw, flags, name = gh.decode_commands(torch, codec, lay, t)
        assert st == 0, (what, st, name)
        gh.assert_command_kernel(fam, name, what)
        gh.assert_raw(raw, lay, streams, what)
        assert not flags.any(), what
    codec.close()


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_segment_path_still_decodes_the_same_batch(fam, sources):
    """no regression of the segment entry point: the same coded bytes with the executor's segments, through a SEG = true instance"""
    import torch
    import divans_amd as da
    g, o, streams, coded, lay = _case(fam, sources)
    t = gh.to_device(torch, lay)
    tin = gh.input_tensors(torch, gh.as_tuples(streams))
    codec = gh.codec_for(da, fam, g, lay["lit_longest"])
    codec.set_geometry(blocks=2)
    st, back, name = gh.decode_segments(torch, codec, dict(tin, longest=lay["lit_longest"]), (t["coded"], t["coded_off"], t["coded_sz"]))
    codec.close()
    mm = fam.mm if fam.mm >= 0 else -1
    assert st == 0 and "lit_decode2_kernel_" in name and f"<{mm}, {gh.tf(fam.ctxc)}, {gh.tf(fam.mix)}, true, " in name, (st, name)
    assert (back == tin["lit"].cpu().numpy()).all()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mixing", [0, 2])
def test_golden_ir_decodes_to_its_expansion(name, mixing):
    import torch
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text(name))
    cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
    ocfg = po.LitConfig.from_buffer_copy(bytes(cfg))
    s = gh.ir_stream(ir, name)
    lay = cc.layout([s], gh.oracle_bytes(ocfg, [s]))
    codec = da.LiteralCodec(cfg, lay["lit_longest"])
    codec.set_block_types(ir.num_block_types)
    st, raw, flags, kname = gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay), with_ins=s["ins"].size > 0)
    codec.close(); ir.close()
    assert st == 0 and "lit_decode2_cmd_kernel" in kname, (st, kname)
    gh.assert_raw(raw, lay, [s], name)
    assert not flags.any()


def test_ragged_batch_of_command_list_prefixes():
    """40 streams, each the first n_k commands of alice29-priors: different lists, raw sizes and literal counts under one configuration"""
    import torch
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text("alice29-priors"))
    cfg = ir.lit_config(dynamic_context_mixing=2)
    ocfg = po.LitConfig.from_buffer_copy(bytes(cfg))
    cmds, ins = ir.device_commands()
    lit, _ = ir.literal_segments()
    streams = cc.prefix_streams(cmds, lit, ins, 40)
    full = ir.expand()
    assert all((s["raw"] == full[:s["raw"].size]).all() for s in streams) and len(set(s["raw"].size for s in streams)) > 30
    lay = cc.layout(streams, gh.oracle_bytes(ocfg, streams))
    codec = da.LiteralCodec(cfg, lay["lit_longest"])
    codec.set_block_types(ir.num_block_types)
    codec.set_geometry(blocks=1)
    st, raw, flags, kname = gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay))
    codec.close(); ir.close()
    assert st == 0, (st, kname)
    gh.assert_raw(raw, lay, streams, "prefixes")
    assert not flags.any()


FAULT_FAMILIES = [f for f in sc.FAMILIES if f.name in ("mm4_const_plain", "mm0_map_plain", "mm4_map_mix", "mmx_map_mix_nocache")]


@pytest.mark.parametrize("fam", FAULT_FAMILIES, ids=repr)
def test_faulty_lists_are_reported_and_contained(fam, sources):
    """every faulty list among good neighbours, one launch each: the right status bit and not the other one, the stream flags name the
    victim alone, the neighbours decode right, no sentinel byte is touched.  The victim's coded bytes are those of its good list."""
    import torch
    import divans_amd as da
    g, o = fam.pair(da, po)
    victim, neighbour = cc.victim_base(fam, sources)
    at = 3
    good = [neighbour, neighbour, neighbour, victim, neighbour, neighbour, neighbour]
    coded = gh.oracle_bytes(o, good)
    codec = gh.codec_for(da, fam, g, 64)
    codec.set_geometry(blocks=1)
    lay = cc.layout(good, coded)
    st, raw, flags, name = gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay))
    assert st == 0 and not flags.any(), (st, name)
    gh.assert_raw(raw, lay, good, "the good list")
    for what, cmds, nlit, bit in cc.faulty_lists(fam, victim):
        batch = list(good)
        batch[at] = dict(victim, cmds=cmds)
        lay = cc.layout(batch, coded, lit_sizes=[nlit if i == at else s["lit"].size for i, s in enumerate(batch)])
        st, raw, flags, name = gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay))
        other = cc.BAD_SEGMENT if bit == cc.BAD_COMMAND else cc.BAD_COMMAND
        assert st & bit and not st & other and not st & ~(bit | cc.BAD_STREAM), (what, st, name)
        assert flags[at] == 1 and int(flags.sum()) == 1, (what, flags[:lay["n"]].tolist())
        gh.assert_raw(raw, lay, batch, what, skip=(at,))
    codec.close()


def test_insert_command_without_insert_bytes_is_a_bad_command(sources):
    """all three insert arrays NULL: the batch has no INSERT commands, and a list that holds one anyway is refused on the device"""
    import torch
    import divans_amd as da
    fam = sc.FAMILIES[0]
    g, o = fam.pair(da, po)
    victim, neighbour = cc.victim_base(fam, sources)
    rng = np.random.default_rng(5)
    plain = cc.Stream("no_inserts", fam, sc._Data(sources, rng), rng).lit(20).copy(9, 4).lit(7).done()
    batch = [plain, victim, plain]
    lay = cc.layout(batch, gh.oracle_bytes(o, batch))
    codec = gh.codec_for(da, fam, g, 64)
    st, raw, flags, name = gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay), with_ins=False)
    codec.close()
    assert st & cc.BAD_COMMAND and not st & cc.BAD_SEGMENT, (st, name)
    assert flags[:3].tolist() == [0, 1, 0]
    gh.assert_raw(raw, lay, batch, "no insert bytes", skip=(1,))


def test_wrap_checked_speed_is_refused(sources):
    """a speed whose row totals leave i16 decodes with generation 1, which has no command-list instances: EINVAL with a message"""
    import torch
    import divans_amd as da
    fam = next(f for f in sc.FAMILIES if f.name == "mm4_const_plain")
    g, o = fam.pair(da, po)
    speed = (0x7800, 0x7800)
    assert not da.speed_supported(*speed) and da.speed_accepted(*speed)
    for i in range(4):
        g.literal_adaptation[i].inc, g.literal_adaptation[i].lim = speed
    victim, neighbour = cc.victim_base(fam, sources)
    lay = cc.layout([neighbour], [np.zeros(16, np.uint8)])
    codec = gh.codec_for(da, fam, g, 64)
    with pytest.raises(da.DivansGpuError, match="command lists need decoder generation 2 or 3"):
        gh.decode_commands(torch, codec, lay, gh.to_device(torch, lay))
    codec.close()
