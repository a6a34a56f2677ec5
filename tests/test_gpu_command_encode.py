"""divans_gpu_lit_encode_commands_batch: general streams encoded from their raw bytes and command lists -- the device derives the
literals and the segment list, verifies that the Copy / Insert commands reproduce the raw bytes and runs the segment encoders.  The
expectation is the C ORACLE's bytes for the segments the Python executor of tests/command_cases.py derived the raw bytes from
(tests/test_command_encode_cases_cpu.py guards them); the contract -- status 0 means the decoder gives the raw bytes back from the
same lists -- is run through divans_gpu_lit_decode_commands_batch.  Every input lies between sentinel bytes and is compared whole
afterwards; the output slots are pre-filled and compared with what the segment call leaves of the same fill."""
import ctypes

import numpy as np
import pytest

import command_cases as cc
import command_encode_cases as ce
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


def _lay(streams):
    """cc.layout with the raw bytes in place (what a compressor hands over): `raw` = `expect`"""
    lay = cc.layout(streams, [np.zeros(0, np.uint8)] * len(streams))
    lay["raw"] = lay["expect"].copy()
    return lay


def _case(fam, sources):
    """the family's configurations, its two batches, the oracle's bytes and the layouts: computed once, shared, never written to"""
    if fam.name not in _CASES:
        import divans_amd as da
        g, o = fam.pair(da, po)
        batches = {}
        for what, streams in (("directed", cc.directed(fam, sources)), ("count_edges", ce.count_edges(fam, sources))):
            batches[what] = (streams, gh.oracle_bytes(o, streams), _lay(streams))
        _CASES[fam.name] = (g, o, batches)
    return _CASES[fam.name]


def _segments_call(torch, codec, streams, cap):
    """divans_gpu_lit_encode_segments_batch on the executor's lists for the same streams, into slots pre-filled the same way"""
    tin = gh.input_tensors(torch, gh.as_tuples(streams))
    outs = gh.encode_outputs(codec, tin["n"])
    st, _, _ = gh.encode_segments(codec, dict(tin, longest=cap), outs)
    o = outs["offsets"].cpu().numpy(); z = outs["sizes"].cpu().numpy()
    return st, outs["out"].cpu().numpy(), [(int(o[i]), int(o[i]) + int(z[i])) for i in range(tin["n"])]


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_directed_batches(fam, sources):
    import torch
    import divans_amd as da
    g, o, batches = _case(fam, sources)
    codec = gh.codec_for(da, fam, g, max(lay["lit_longest"] for _, _, lay in batches.values()))      # one codec: one allocation of the tables
    paths = gh.encode_paths(codec, da)
    for which, (streams, coded, lay) in batches.items():
        t = gh.to_device(torch, lay)
        for path in paths:
            what = f"{which}, path {path}"
            codec.set_encode_path(path)
            res = gh.encode_commands(torch, codec, lay, t)
            assert res["status"] == 0 and not res["flags"].any(), (what, res["status"], res["flags"].tolist())
            assert codec.last_encode_path() == 1 if path == 1 else codec.last_encode_path() in (2, 3), (what, codec.last_encode_path())
            gh.assert_coded(res, streams, coded, what)
            # what the segment call leaves of the fill outside the coded streams, this call leaves too
            st, seg_out, seg_spans = _segments_call(torch, codec, streams, lay["lit_longest"])
            assert st == 0 and seg_spans == res["spans"], what
            outside = np.ones(seg_out.size, bool)
            for b, e in seg_spans:
                outside[b:e] = False
            kept = outside & (seg_out == gh.OUT_SENTINEL)
            assert (res["out"][kept] == gh.OUT_SENTINEL).all(), f"{what}: slot bytes overwritten that the segment call leaves alone"
    codec.close()


def test_one_stream(sources):
    import torch
    import divans_amd as da
    fam = next(f for f in sc.FAMILIES if f.name == "mm4_map_mix")
    g, o, batches = _case(fam, sources)
    streams, coded, _ = batches["directed"]
    k = next(i for i, s in enumerate(streams) if s["name"] == "lit1to17_each_then_copy")
    lay = _lay([streams[k]])
    codec = gh.codec_for(da, fam, g, lay["lit_longest"])
    res = gh.encode_commands(torch, codec, lay, gh.to_device(torch, lay))
    codec.close()
    assert res["status"] == 0 and not res["flags"].any()
    gh.assert_coded(res, [streams[k]], [coded[k]], "one stream")


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=repr)
def test_round_trip_through_the_command_decoder(fam, sources):
    """the contract: the GPU's coded bytes (re-laid at 4-byte offsets) and its d_lit_sizes, with the same lists, decode to the raw bytes"""
    import torch
    import divans_amd as da
    g, o, batches = _case(fam, sources)
    codec = gh.codec_for(da, fam, g, max(lay["lit_longest"] for _, _, lay in batches.values()))
    codec.set_geometry(blocks=2)        # tables of 32 streams, not of a full grid; every group codes and decodes several streams in a row
    for which, (streams, coded, lay) in batches.items():
        res = gh.encode_commands(torch, codec, lay, gh.to_device(torch, lay))
        assert res["status"] == 0, (which, res["status"])
        gh.round_trip_commands(torch, codec, streams, res, lay, which)
    codec.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mixing", [0, 2])
def test_golden_ir_codes_as_its_segments(name, mixing):
    import torch
    import divans_amd as da
    ir = da.CommandIR(irtext.load_ir_text(name))
    cfg = ir.lit_config(dynamic_context_mixing=mixing, use_context_map=1)
    ocfg = po.LitConfig.from_buffer_copy(bytes(cfg))
    s = gh.ir_stream(ir, name)
    lay = _lay([s])
    codec = da.LiteralCodec(cfg, lay["lit_longest"])
    codec.set_block_types(ir.num_block_types)
    res = gh.encode_commands(torch, codec, lay, gh.to_device(torch, lay), with_ins=s["ins"].size > 0)
    st, seg_out, seg_spans = _segments_call(torch, codec, [s], lay["lit_longest"])
    codec.close(); ir.close()
    assert res["status"] == 0 and st == 0 and not res["flags"].any(), (res["status"], st)
    b, e = seg_spans[0]
    assert res["spans"] == seg_spans and (res["coded"][0] == seg_out[b:e]).all(), "differs from encode_segments_batch on literal_segments()"
    gh.assert_coded(res, [s], gh.oracle_bytes(ocfg, [s]), name)


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
    lay = _lay(streams)
    codec = da.LiteralCodec(cfg, lay["lit_longest"])
    codec.set_block_types(ir.num_block_types)
    res = gh.encode_commands(torch, codec, lay, gh.to_device(torch, lay))
    codec.close(); ir.close()
    assert res["status"] == 0 and not res["flags"].any(), res["status"]
    gh.assert_coded(res, streams, gh.oracle_bytes(ocfg, streams), "prefixes")


FAULT_FAMILIES = [f for f in sc.FAMILIES if f.name in ("mm4_const_plain", "mm0_map_plain", "mm4_map_mix", "mmx_map_mix_nocache")]


@pytest.mark.parametrize("fam", FAULT_FAMILIES, ids=repr)
def test_faulty_inputs_are_reported_and_contained(fam, sources):
    """every faulty input as the middle stream between good neighbours, one call each: the listed bit and not the other one, the flag
    on the victim alone, d_lit_sizes[victim] = 0, the victim coded as a stream without literals, the neighbours as the oracle codes
    them, nothing written outside the slots (asserted inside gpu_harness.encode_commands).  The two inputs that must pass raise nothing."""
    import torch
    import divans_amd as da
    g, o = fam.pair(da, po)
    victim, _ = cc.victim_base(fam, sources)
    rng = np.random.default_rng(99700 + fam.seed)       # neighbours with fewer literals than any lit_stream_len below: the cap is the batch's
    neighbour = cc.Stream("neighbour", fam, sc._Data(sources, rng), rng).lit(20).copy(9, 4).ins(3).lit(7).copy(5, 30).done()
    at = 1
    none = sc.segments([], [], [])
    empty = po.lit_segments_encode(o, np.zeros(0, np.uint8), none["len"], none["btype"], none["last8"])
    ref_neighbour = gh.oracle_bytes(o, [neighbour])[0]
    codec = gh.codec_for(da, fam, g, 128)
    for e in ce.faulty_inputs(fam, victim, sources):
        middle = dict(name=e["what"], cmds=e["cmds"], raw=e["raw"], ins=e["ins"], lit=e["lit"] if e["lit"] is not None else np.zeros(0, np.uint8),
                      segs=e["segs"] if e["segs"] is not None else sc.segments([], [], []))
        batch = [neighbour, middle, neighbour]
        lay = _lay(batch)
        res = gh.encode_commands(torch, codec, lay, gh.to_device(torch, lay), lit_cap=e["lit_cap"])
        st, bit = res["status"], e["bit"]
        if bit:
            other = cc.BAD_SEGMENT if bit == cc.BAD_COMMAND else cc.BAD_COMMAND
            assert st & bit and not st & other and not st & ~bit, (e["what"], st)
            assert res["flags"].tolist() == [0, 1, 0], (e["what"], res["flags"].tolist())
            assert int(res["lit_sz"][at]) == 0, e["what"]
            assert res["coded"][at].size == empty.size and (res["coded"][at] == empty).all(), e["what"]
            gh.assert_coded(res, batch, [ref_neighbour, None, ref_neighbour], e["what"], skip=(at,))
        else:
            assert st == 0 and not res["flags"].any(), (e["what"], st, res["flags"].tolist())
            gh.assert_coded(res, batch, [ref_neighbour, gh.oracle_bytes(o, [middle])[0], ref_neighbour], e["what"])
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
    lay = _lay(batch)
    codec = gh.codec_for(da, fam, g, 64)
    res = gh.encode_commands(torch, codec, lay, gh.to_device(torch, lay), with_ins=False)
    codec.close()
    assert res["status"] == cc.BAD_COMMAND and res["flags"].tolist() == [0, 1, 0] and int(res["lit_sz"][1]) == 0, (res["status"], res["flags"].tolist())
    ref = gh.oracle_bytes(o, [plain])[0]
    gh.assert_coded(res, batch, [ref, None, ref], "no insert bytes", skip=(1,))


def test_refusals(sources):
    import torch
    import divans_amd as da
    fam = sc.FAMILIES[0]
    g, o = fam.pair(da, po)
    victim, neighbour = cc.victim_base(fam, sources)
    lay = _lay([neighbour, victim])
    t = gh.to_device(torch, lay)
    codec = gh.codec_for(da, fam, g, 64)
    L, h = codec._lib, codec._h
    outs = gh.encode_outputs(codec, 2)
    lit_sz = torch.zeros(2, dtype=torch.int32, device=t["raw"].device)
    args = [t["raw"], t["raw_off"], t["raw_sz"], 2, t["cmd_begin"], t["cmds"], 64, t["ins"], t["ins_off"], t["ins_sz"], outs["out"], outs["slot"], outs["offsets"],
            outs["sizes"], lit_sz]
    ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a

    def call(edit):
        a = list(args)
        for k, v in edit.items():
            a[k] = v
        return L.divans_gpu_lit_encode_commands_batch(h, *[ptr(x) for x in a])
    assert call({}) == 0 and codec.status() == 0
    for k in (0, 1, 2, 4, 5, 10, 12, 13, 14):                      # every pointer but the insert triple
        assert call({k: None}) == -1, k
    assert L.divans_gpu_lit_encode_commands_batch(None, *[ptr(x) for x in args]) == -1
    for gone in ((7,), (8,), (9,), (7, 8), (8, 9), (7, 9)):        # an incomplete insert triple
        assert call({k: None for k in gone}) == -1, gone
    assert call({6: 65}) == -1                                     # lit_stream_len above max_stream_len
    assert call({11: outs["slot"] - 16}) == -4 and call({11: outs["slot"] + 8}) == -4      # DIVANS_GPU_ECAP, as the segment call
    with pytest.raises(da.DivansGpuError, match="out_slot"):
        codec.encode_segments_batch(t["raw"], t["raw_off"], t["raw_sz"], 2, 64, t["cmd_begin"], t["cmds"], dict(outs, slot=outs["slot"] - 16))
    assert L.divans_gpu_lit_stream_begin(h) == 0
    piece = np.arange(40, dtype=np.uint8); buf = np.zeros(4096, np.uint8); cs = np.zeros(4, np.uint32)
    nch = ctypes.c_uint32(0); got = ctypes.c_size_t(0)
    assert L.divans_gpu_lit_stream_encode(h, piece.ctypes.data, piece.size, 0, buf.ctypes.data, buf.size, cs.ctypes.data, 4, ctypes.byref(nch), ctypes.byref(got)) == 0
    assert call({}) == -1 and b"call by call" in L.divans_gpu_last_error()      # a stream coded call by call is open
    assert L.divans_gpu_lit_stream_finish(h, buf.ctypes.data, buf.size, ctypes.byref(got)) == 0
    codec.close()
