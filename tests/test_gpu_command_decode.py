"""divans_gpu_lit_decode_commands_batch: general streams decoded from their command lists, the decoder running the Copy / Insert
commands itself and taking every Literal command's context from its own output.  The coded bytes are the C ORACLE's (made from the
segments the Python executor of tests/command_cases.py derives; tests/test_command_cases_cpu.py guards both), the expectation is
the executor's raw bytes inside a buffer of sentinels, compared whole.

Two long streams carry the rANS chunk seam: one cannot hold both a command boundary exactly on literal 32 768 and a Literal command
that spans it."""
import numpy as np
import pytest

import command_cases as cc
import irtext
import pyoracle as po
import segment_cases as sc

pytestmark = pytest.mark.gpu
NAMES = ["alice29", "alice29-q11", "alice29-priors", "asyoulik", "random_then_unicode", "ends_with_truncated_dictionary"]
_CASES = {}


@pytest.fixture(scope="module")
def sources(corpus, random_then_unicode, shuffle384):
    return (corpus, random_then_unicode, shuffle384)


def _code(ocfg, streams):
    return [po.lit_segments_encode(ocfg, s["lit"], s["segs"]["len"], s["segs"]["btype"], s["segs"]["last8"]) for s in streams]


def _case(fam, sources):
    """the family's configurations, its directed batch, the oracle's bytes and the batch's layout: computed once, shared, never written to"""
    if fam.name not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        streams = cc.directed(fam, sources)
        coded = _code(o, streams)
        _CASES[fam.name] = (g, o, streams, coded, cc.layout(streams, coded))
    return _CASES[fam.name]


def _tensors(torch, lay):
    dev = torch.device("cuda")
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in lay.items() if isinstance(v, np.ndarray)}


def _decode(torch, codec, lay, t, with_ins=True):
    """-> (status, the whole raw buffer, stream flags, name of the kernel that ran)"""
    raw = t["raw"].clone()
    flags = torch.zeros(lay["n"] + 16, dtype=torch.uint8, device=raw.device)
    codec.set_stream_flags(flags)
    ins = (t["ins"], t["ins_off"], t["ins_sz"]) if with_ins else (None, None, None)
    codec.decode_commands_batch(t["coded"], t["coded_off"], t["coded_sz"], lay["n"], t["cmd_begin"], t["cmds"], t["lit_sz"], lay["lit_longest"],
                                raw, t["raw_off"], t["raw_sz"], *ins)
    st = codec.status()
    codec.set_stream_flags(None)
    return st, raw.cpu().numpy(), flags.cpu().numpy(), codec.last_decode_kernel()


def _b(v):
    return "true" if v else "false"


def _assert_kernel(fam, name, what):
    """lit_decode2_cmd_kernel<MM, CTXC, MIX, caches>: the high-row caches in the 2-way organisation (1 | 16, with mixing 1 | 2 | 16), or none"""
    mm = fam.mm if fam.mm >= 0 else -1
    caches = (19 if fam.mix else 17) if fam.cached else 0
    assert name == f"divans_hip::lit_decode2_cmd_kernel<{mm}, {_b(fam.ctxc)}, {_b(fam.mix)}, {caches}>", (what, name)


def _assert_raw(got, lay, streams, what, skip=()):
    """the whole raw buffer against the expectation, sentinels included (the raw ranges of the streams in `skip` left out)"""
    same = got == lay["expect"]
    for i in skip:
        ro = int(lay["raw_off"][i]); same[ro:ro + int(lay["raw_sz"][i])] = True
    if same.all():
        return
    at = int(np.argmin(same))
    inside = [i for i in range(lay["n"]) if int(lay["raw_off"][i]) <= at < int(lay["raw_off"][i]) + int(lay["raw_sz"][i])]
    if inside:
        i = inside[0]
        raise AssertionError(f"{what}: stream {i} ({streams[i]['name']}, {int(lay['raw_sz'][i])} raw bytes) wrong from its byte {at - int(lay['raw_off'][i])}")
    raise AssertionError(f"{what}: sentinel byte {at} of the raw buffer overwritten with {int(got[at])}")


def _codec(da, fam, g, longest):
    codec = da.LiteralCodec(g, max(longest, 16))
    codec.set_block_types(fam.n_btypes)
    return codec


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_directed_batch(fam, sources):
    """grids of two workgroups and of one (16 resident groups: every group runs two or three streams in a row, so cursor, raw position and
    word ring are reset), then the codec's own grid, and once under a cache organisation the commands call has to reduce"""
    import torch
    import divans_amd as da
    g, o, streams, coded, lay = _case(fam, sources)
    t = _tensors(torch, lay)
    codec = _codec(da, fam, g, lay["lit_longest"])
    steps = [("2 workgroups", lambda c: c.set_geometry(blocks=2)), ("1 workgroup", lambda c: c.set_geometry(blocks=1)),
             ("direct-mapped decoder asked for", lambda c: c.set_decoder(2))]
    if fam.cached:
        steps.append(("tiny 2-way caches with low-row caches asked for", lambda c: c.set_decoder(3, (8, 8, 8, 8), (5, 5, 5, 5), blocks=2)))
    for what, setup in steps:
        setup(codec)
        st, raw, flags, name = _decode(torch, codec, lay, t)
        assert st == 0, (what, st, name)
        _assert_kernel(fam, name, what)
        _assert_raw(raw, lay, streams, what)
        assert not flags.any(), what
    codec.close()


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_segment_path_still_decodes_the_same_batch(fam, sources):
    """no regression of the segment entry point: the same coded bytes with the executor's segments, through a SEG = true instance"""
    import torch
    import divans_amd as da
    g, o, streams, coded, lay = _case(fam, sources)
    dev = torch.device("cuda")
    t = _tensors(torch, lay)
    sizes = np.array([s["lit"].size for s in streams], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(sizes[:-1].astype(np.int64))]).astype(np.int64)
    segs = np.concatenate([s["segs"] for s in streams] + [np.zeros(1, sc.SEG_DTYPE)])
    seg_begin = np.concatenate([[0], np.cumsum([s["segs"].size for s in streams])]).astype(np.int32)
    lit = np.concatenate([s["lit"] for s in streams] + [np.zeros(64, np.uint8)])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    back = torch.zeros(lit.size, dtype=torch.uint8, device=dev)
    codec = _codec(da, fam, g, lay["lit_longest"])
    codec.set_geometry(blocks=2)
    codec.decode_segments_batch(t["coded"], t["coded_off"], t["coded_sz"], len(streams), lay["lit_longest"], d(seg_begin), d(segs.view(np.uint8)), back, d(offs), d(sizes))
    st = codec.status(); name = codec.last_decode_kernel()
    codec.close()
    mm = fam.mm if fam.mm >= 0 else -1
    assert st == 0 and "lit_decode2_kernel_" in name and f"<{mm}, {_b(fam.ctxc)}, {_b(fam.mix)}, true, " in name, (st, name)
    assert (back.cpu().numpy() == lit).all()


def _ir_stream(ir, name):
    cmds, ins = ir.device_commands()
    lit, segs = ir.literal_segments()
    return dict(name=name, cmds=cmds, lit=lit, ins=ins, raw=ir.expand(), segs=segs)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mixing", [0, 2])
def test_golden_ir_decodes_to_its_expansion(name, mixing):
    import torch
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text(name))
    cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
    ocfg = po.LitConfig.from_buffer_copy(bytes(cfg))
    s = _ir_stream(ir, name)
    lay = cc.layout([s], _code(ocfg, [s]))
    codec = da.LiteralCodec(cfg, lay["lit_longest"])
    codec.set_block_types(ir.num_block_types)
    st, raw, flags, kname = _decode(torch, codec, lay, _tensors(torch, lay), with_ins=s["ins"].size > 0)
    codec.close(); ir.close()
    assert st == 0 and "lit_decode2_cmd_kernel" in kname, (st, kname)
    _assert_raw(raw, lay, [s], name)
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
    lay = cc.layout(streams, _code(ocfg, streams))
    codec = da.LiteralCodec(cfg, lay["lit_longest"])
    codec.set_block_types(ir.num_block_types)
    codec.set_geometry(blocks=1)
    st, raw, flags, kname = _decode(torch, codec, lay, _tensors(torch, lay))
    codec.close(); ir.close()
    assert st == 0, (st, kname)
    _assert_raw(raw, lay, streams, "prefixes")
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
    coded = _code(o, good)
    codec = _codec(da, fam, g, 64)
    codec.set_geometry(blocks=1)
    lay = cc.layout(good, coded)
    st, raw, flags, name = _decode(torch, codec, lay, _tensors(torch, lay))
    assert st == 0 and not flags.any(), (st, name)
    _assert_raw(raw, lay, good, "the good list")
    for what, cmds, nlit, bit in cc.faulty_lists(fam, victim):
        batch = list(good)
        batch[at] = dict(victim, cmds=cmds)
        lay = cc.layout(batch, coded, lit_sizes=[nlit if i == at else s["lit"].size for i, s in enumerate(batch)])
        st, raw, flags, name = _decode(torch, codec, lay, _tensors(torch, lay))
        other = cc.BAD_SEGMENT if bit == cc.BAD_COMMAND else cc.BAD_COMMAND
        assert st & bit and not st & other and not st & ~(bit | cc.BAD_STREAM), (what, st, name)
        assert flags[at] == 1 and int(flags.sum()) == 1, (what, flags[:lay["n"]].tolist())
        _assert_raw(raw, lay, batch, what, skip=(at,))
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
    lay = cc.layout(batch, _code(o, batch))
    codec = _codec(da, fam, g, 64)
    st, raw, flags, name = _decode(torch, codec, lay, _tensors(torch, lay), with_ins=False)
    codec.close()
    assert st & cc.BAD_COMMAND and not st & cc.BAD_SEGMENT, (st, name)
    assert flags[:3].tolist() == [0, 1, 0]
    _assert_raw(raw, lay, batch, "no insert bytes", skip=(1,))


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
    codec = _codec(da, fam, g, 64)
    with pytest.raises(da.DivansGpuError, match="command lists need decoder generation 2 or 3"):
        _decode(torch, codec, lay, _tensors(torch, lay))
    codec.close()
